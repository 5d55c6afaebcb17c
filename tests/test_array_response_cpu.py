"""Host side of the array response (no GPU): the steering header (``d2d_steer.hpp``) through a plain g++ build against its NumPy
restatement (bit for bit, the clamp included), the host's parameter and memory checks through ctypes and through a stand-alone g++
program, plain and with sanitizers, the oracle recipe of ``tests/array_response_oracle.py`` against the coherent field's (which the GPU
tests then hold the kernel to), ``utils.ula`` / ``channel_matrix`` / ``beamformed_power`` / ``singular_values`` / ``mimo_capacity``
against closed forms, and the bindings."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import coherent_field_oracle as CFO
from array_response_oracle import (AMP_LINEAR, AMP_SQRT, ARRAY_MAX, ArrayResponse, fold, physics, steer_dot, steer_inputs, steer_phase,
                                   unit_dir)
from conftest import unit_grid
from test_gpu_power_angle import _directed
from test_gpu_strongest_paths import _case, _contributions

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "array_response_host.cpp")
GXX = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]
INV_20 = F(1) / F(0.05)
WL = 0.05


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """d2d_steer.hpp and d2d_host.hpp's array checks, compiled for the host (tests/native/array_response_host.cpp)."""
    so = str(tmp_path_factory.mktemp("ar_host") / "libar_host.so")
    subprocess.check_call(GXX + ["-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    fp = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    bp = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
    lib.ar_unit_dir.argtypes = [C.c_longlong, fp, fp, fp, fp, bp]
    lib.ar_unit_dir.restype = None
    lib.ar_steer_dot.argtypes = [C.c_longlong, fp, fp, fp, fp, fp]
    lib.ar_steer_dot.restype = None
    lib.ar_steer_phase.argtypes = [C.c_longlong, fp, fp, fp, fp, fp]
    lib.ar_steer_phase.restype = None
    lib.ar_array_params.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int, C.POINTER(C.c_int)]
    lib.ar_array_params.restype = C.c_int
    lib.ar_bytes_per_cell.argtypes = [C.c_int, C.c_int]
    lib.ar_bytes_per_cell.restype = C.c_longlong
    lib.ar_array_fits.argtypes = [C.c_ulonglong, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong]
    lib.ar_array_fits.restype = C.c_int
    return lib


def host_unit_dir(host, dx, dy):
    dx, dy = np.ascontiguousarray(dx, F), np.ascontiguousarray(dy, F)
    ux, uy, ok = np.empty_like(dx), np.empty_like(dx), np.empty(dx.size, np.uint8)
    host.ar_unit_dir(dx.size, dx, dy, ux, uy, ok)
    return ux, uy, ok.astype(bool)


def host_steer_phase(host, f0, qt, qr, inv):
    a = [np.ascontiguousarray(v, F) for v in (f0, qt, qr, inv)]
    out = np.empty_like(a[0])
    host.ar_steer_phase(out.size, *a, out)
    return out


# ---- the steering header -----------------------------------------------------------------------------------------------------------
def test_steer_header_equals_its_numpy_restatement_bit_for_bit(host):
    dx, dy, f0, qt, qr, inv = steer_inputs()
    assert dx.size > 2 * 10**5
    ux, uy, ok = host_unit_dir(host, dx, dy)
    wx, wy, wok = unit_dir(dx, dy)
    assert np.array_equal(ok, wok) and ok.sum() > 2 * 10**5 and (~ok).sum() > 300
    # zero, denormal, huge and non-finite directions are all in the set, and none of them has a unit vector
    for d in [(0, 0), (-0.0, 0), (-0.0, -0.0), (np.nextafter(F(0), F(1)),) * 2, (1e-30, 1e-30), (1e30, 1), (np.finfo(F).max,) * 2, (np.nan, 1), (1, -np.inf)]:
        at = (_bits(dx) == _bits(F(d[0]))) & (_bits(dy) == _bits(F(d[1])))
        assert at.any() and not ok[at].any(), d
    # (where there is none the divisions' results are not used: they are compared all the same, NaN as NaN)
    for name, got, want in (("ux", ux, wx), ("uy", uy, wy)):
        same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), f"{name}: {(~same).sum()} differ, first at ({dx[~same][0]!r}, {dy[~same][0]!r})"
    assert np.abs(np.hypot(ux[ok].astype(np.float64), uy[ok].astype(np.float64)) - 1).max() < 4 * 2.0**-24
    # steer_dot with the unit vectors of the set (offsets: qt and qr of the set, which include -0.0)
    q = np.empty_like(dx)
    host.ar_steer_dot(dx.size, qt, qr, np.where(ok, ux, F(0.6)), np.where(ok, uy, F(0.8)), q)
    with np.errstate(all="ignore"):
        wq = np.asarray(qt * np.where(ok, ux, F(0.6)) + qr * np.where(ok, uy, F(0.8)), F)
    assert np.array_equal(_bits(q)[~np.isnan(wq)], _bits(wq)[~np.isnan(wq)]) and np.array_equal(np.isnan(q), np.isnan(wq))
    assert np.array_equal(_bits(steer_dot(qt[7], qr[7], ux[ok], uy[ok])), _bits(qt[7] * ux[ok] + qr[7] * uy[ok]))
    # steer_phase
    f = host_steer_phase(host, f0, qt, qr, inv)
    wf = steer_phase(f0, qt, qr, inv)
    nan = np.isnan(wf)
    assert np.array_equal(np.isnan(f), nan) and nan.sum() > 100
    bad = _bits(f)[~nan] != _bits(wf)[~nan]
    assert not bad.any(), f"steer_phase: {bad.sum()} differ"
    assert (f[~nan] >= 0).all() and (f[~nan] < 1).all()
    # offsets of -0.0 are in the set and leave f0 as it is
    z = (_bits(qt) == _bits(F(-0.0))) & (_bits(qr) == _bits(F(-0.0))) & ~np.isnan(f0)
    assert z.any() and np.array_equal(_bits(f[z]), _bits(f0[z]))


def test_the_clamp_fires_where_the_subtraction_rounds_to_one(host):
    """f0 = 0 and w = 1e-9: v = -1e-9, floorf(v) = -1, v + 1 rounds to 1.0f -- outside the phasor's [0, 1).  The clamp takes it to 0,
    the same point of the circle.  Without it the case would be outside phasor's input range."""
    with np.errstate(all="ignore"):
        v = F(0) - F(1e-9)
        assert v - np.floor(v) == F(1)  # what the clamp is there for
    for f0, qt, qr, inv in [(0, 1e-9, 0, 1), (0, 0, 1e-9, 1), (0, 5e-11, 0, 20), (0, np.nextafter(F(0), F(1)), 0, 1)]:
        args = [np.array([x], F) for x in (f0, qt, qr, inv)]
        got = host_steer_phase(host, *args)
        assert _bits(got)[0] == 0 and _bits(steer_phase(*args))[0] == 0, (f0, qt, qr, inv)
    # its neighbours are not clamped
    below1 = np.nextafter(F(1), F(0))
    got = host_steer_phase(host, *[np.array(x, F) for x in ([0, 0, below1], [-1e-9, 3e-8, 0], [0, 0, 0], [1, 1, 1])])
    assert got[0] == F(1e-9) and got[1] == below1 and got[2] == below1
    c, s = CFO.phasor(np.array([0], F))
    assert c[0] == 1 and _bits(s)[0] == 0


# ---- the host's share of the launch ----------------------------------------------------------------------------------------------
def _params(host, tx, rx, inv=20.0, amp=0, nt=None, nr=None):
    tx, rx = (None if e is None else np.ascontiguousarray(e, F).reshape(-1, 2) for e in (tx, rx))
    at = C.c_int(-7)
    rc = host.ar_array_params(len(tx) if nt is None else nt, None if tx is None else tx.ctypes.data, len(rx) if nr is None else nr,
                              None if rx is None else rx.ctypes.data, inv, amp, C.byref(at))
    return rc, at.value


def test_array_params_on_every_bad_position_and_both_limits_of_both_counts(host):
    assert ARRAY_MAX == 8
    for nt in (1, ARRAY_MAX):
        for nr in (1, ARRAY_MAX):
            tx, rx = np.full((nt, 2), 0.025, F), np.full((nr, 2), -0.0, F)
            assert _params(host, tx, rx) == (0, -1) and _params(host, tx, rx, 0.0, 1) == (0, -1)
            for bad in (np.nan, np.inf, -np.inf):
                for k in range(2 * nt):
                    t2 = tx.copy()
                    t2.reshape(-1)[k] = bad
                    assert _params(host, t2, rx) == (-1, k // 2), (nt, nr, k, bad)
                for k in range(2 * nr):
                    r2 = rx.copy()
                    r2.reshape(-1)[k] = bad
                    assert _params(host, tx, r2) == (-1, k // 2), (nt, nr, k, bad)
    # counts out of range: refused without reading a list (there is none)
    for bad in (0, -1, ARRAY_MAX + 1, 2**30, -(2**30)):
        assert _params(host, None, None, nt=bad, nr=1) == (-1, -1)
        assert _params(host, None, None, nt=1, nr=bad) == (-1, -1)
    one = np.zeros((1, 2), F)
    for inv in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert _params(host, one, one, inv) == (-1, -1)
    for amp in (2, -1):
        assert _params(host, one, one, 20.0, amp) == (-1, -1)


def test_array_fits_at_the_boundary_byte_and_with_sizes_that_would_wrap(host):
    assert [host.ar_bytes_per_cell(*p) for p in ((1, 1), (4, 3), (4, 4), (8, 8))] == [12, 100, 132, 516]
    top = 2**64 - 1
    for mem_free in (0, 2**20, 3 * 2**30, 288 * 2**30, top):
        for held in (0, 2**16, 5 * 2**30, top):
            for nt, nr in ((1, 1), (4, 3), (8, 8)):
                per = 8 * nt * nr + 4
                budget = mem_free // 2 + held // 2
                edge = budget // per
                assert host.ar_array_fits(edge, nt, nr, mem_free, held) == 1 and host.ar_array_fits(edge + 1, nt, nr, mem_free, held) == 0
                # the boundary byte: one cell more fits exactly when the budget grows to hold it
                if mem_free == 288 * 2**30 and held == 0:
                    need = (edge + 1) * per  # bytes
                    assert host.ar_array_fits(edge + 1, nt, nr, 2 * need, 0) == 1 and host.ar_array_fits(edge + 1, nt, nr, 2 * need - 2, 0) == 0
    # 2 * 10^9 cells of an 8 x 8 matrix: over a terabyte (what no quick GPU test can hold)
    assert host.ar_array_fits(2 * 10**9, 8, 8, 288 * 2**30, 0) == 0 and host.ar_array_fits(1024 * 1024, 8, 8, 200 * 2**30, 0) == 1
    # cells * bytes per cell wraps 64 bits: still refused
    assert (top // 516 + 2) * 516 >= 2**64
    assert host.ar_array_fits(top // 516 + 2, 8, 8, 288 * 2**30, 0) == 0 and host.ar_array_fits(top, 8, 8, 288 * 2**30, 0) == 0
    assert host.ar_array_fits(top // 12 + 2, 1, 1, top, top) == 0 and host.ar_array_fits(2**62, 1, 1, 2**40, 0) == 0


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_stand_alone_host_program(tmp_path, sanitize):
    """array_params, array_fits (refusals included) and the header's exact cases in a program of their own; with sanitizers it is the
    same program, linked against the sanitizers' run times by the compiler (nothing is preloaded, nothing is loaded into Python)."""
    exe = str(tmp_path / "ar_host")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(GXX + extra + ["-DAR_MAIN", "-o", exe, SRC])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(done.stdout)
    assert done.returncode == 0, done.stdout
    assert "array_response_host: 0 failures" in done.stdout


# ---- the oracle recipe ---------------------------------------------------------------------------------------------------------------
def _joined(scene, mode, role):
    _, T, Rl, _ = _contributions(scene, mode, role, "received_power")
    _, T2, D = _directed(scene, mode, role, "received_power")
    assert np.array_equal(T.view(np.uint32), T2.view(np.uint32))  # the two oracles' contributions agree in bits
    return T, Rl, D


@pytest.mark.parametrize("amp", [AMP_SQRT, AMP_LINEAR], ids=["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle", "square_centre"])
def test_zero_offset_pair_is_the_coherent_field_recipe_by_bits(scene, mode, role, amp):
    """A pair whose two offsets are (+-0, +-0) is the coherent field wherever no contribution lacks a direction: every cell of random7
    and obstacle; in square_centre the line of sight of the cell that IS the fixed end point has none, and exactly [4, 4] differs."""
    T, Rl, D = _joined(scene, mode, role)
    etx = np.array([[0.0, -0.0], [0.03, 0.01]], F)
    erx = np.array([[0.02, -0.07], [-0.0, 0.0], [-0.0, -0.0]], F)
    re, im, total = fold(T, Rl, D, INV_20, amp, etx, erx)
    cre, cim, ctotal = CFO.fold(T, Rl, INV_20, amp)
    assert np.array_equal(_bits(total), _bits(ctotal))
    _, _, okt = unit_dir(D[:, :, 0], D[:, :, 1])
    _, _, okr = unit_dir(D[:, :, 2], D[:, :, 3])
    lacking = ((T != 0) & ~(okt & okr)).any(axis=0)
    shape = _case(scene)[2].shape
    if scene == "square_centre":
        assert np.argwhere(lacking.reshape(shape)).tolist() == [[4, 4]]
    else:
        assert not lacking.any()
    for i in (1, 2):
        dre, dim = _bits(re[i, 0]) != _bits(cre), _bits(im[i, 0]) != _bits(cim)
        if scene == "square_centre":
            assert np.argwhere(dre.reshape(shape)).tolist() == [[4, 4]] and np.argwhere((dre | dim).reshape(shape)).tolist() == [[4, 4]]
        else:
            assert not dre.any() and not dim.any()
    assert np.count_nonzero(cim) > cim.size // 3
    # the planes off the origin differ from it and from each other in bits
    planes = [(re[i, j], im[i, j]) for i in range(2) for j in range(2)]
    for a in range(len(planes)):
        for b in range(a + 1, len(planes)):
            assert not np.array_equal(_bits(planes[a][1]), _bits(planes[b][1])), (a, b)


def test_recipe_entries_depend_on_their_own_elements_only_and_meet_the_physics():
    T, Rl, D = _joined("random7", "hsig", "rx")
    etx = np.array([[0.0, 0.0], [0.025, 0.0], [0.0, -0.1], [0.07, 0.04]], F)
    erx = np.array([[0.01, 0.02], [-0.05, 0.0], [0.0, 0.09]], F)
    re, im, total = fold(T, Rl, D, INV_20, AMP_SQRT, etx, erx)
    pt, pr = [2, 0, 3, 1], [1, 2, 0]
    re2, im2, total2 = fold(T, Rl, D, INV_20, AMP_SQRT, etx[pt], erx[pr])
    assert np.array_equal(_bits(re2), _bits(re[pr][:, pt])) and np.array_equal(_bits(im2), _bits(im[pr][:, pt]))
    re3, im3, _ = fold(T, Rl, D, INV_20, AMP_SQRT, etx[[1, 1]], erx[:2])
    assert np.array_equal(_bits(re3[:, 0]), _bits(re3[:, 1])) and np.array_equal(_bits(re3[:, 0]), _bits(re[:2, 1]))
    assert np.array_equal(_bits(im3[:, 1]), _bits(im[:2, 1])) and np.array_equal(_bits(total2), _bits(total))
    H, bound = physics(T, Rl, D, INV_20, AMP_SQRT, etx, erx)
    err = np.abs(re.astype(np.float64) + 1j * im.astype(np.float64) - H)
    lit = bound > 0
    print(f"max error / bound {np.max(err[lit] / bound[lit]):.3f}")
    assert lit.mean() > 1 / 3 and (err <= bound).all() and (np.abs(H.imag) > 0).mean() > 1 / 3
    # the steering is physics, not decoration: an element half a wavelength towards a line-of-sight path turns its phase by pi
    H0 = H[:, 0]
    assert np.abs(H[:, 1] - H0).max() > 0.1 * np.abs(H0).max()


def test_recipe_from_the_walls_on_a_grid_of_its_own():
    """array_response() end to end (what the GPU tests call for a grid they have no cached contributions of): the zero-offset pair
    is coherent_field() of the same scene by bits, total included."""
    from array_response_oracle import array_response

    walls, fixed, _, _ = _case("random7")
    X, Y = unit_grid(7, 5)
    kw = dict(min_order=0, max_order=2, approx=True, function="hard_sigmoid")
    etx, erx = np.array([[0.0, 0.0], [0.01, 0.03]], F), np.array([[-0.0, 0.0]], F)
    ar = array_response(walls, fixed, X, Y, INV_20, AMP_LINEAR, etx, erx, **kw)
    cf = CFO.coherent_field(walls, fixed, X, Y, INV_20, AMP_LINEAR, **kw)
    assert ar.re.shape == ar.im.shape == (1, 2, 5, 7) and ar.total.shape == (5, 7)
    assert np.array_equal(_bits(ar.re[0, 0]), _bits(cf.re)) and np.array_equal(_bits(ar.im[0, 0]), _bits(cf.im))
    assert np.array_equal(_bits(ar.total), _bits(cf.total)) and cf.im.any() and not np.array_equal(_bits(ar.im[0, 1]), _bits(cf.im))


# ---- utils ---------------------------------------------------------------------------------------------------------------------------
def test_ula_is_centred_and_oriented():
    from differt2d_amd.utils import ula

    e = ula(4, 0.025)
    assert e.dtype == F and e.shape == (4, 2)
    assert np.array_equal(e, np.array([[-0.0375, 0], [-0.0125, 0], [0.0125, 0], [0.0375, 0]], F))
    assert np.array_equal(ula(1, 0.5), np.zeros((1, 2), F))
    v = ula(3, 2.0, np.pi / 2)
    assert np.allclose(v, [[0, -2], [0, 0], [0, 2]], atol=1e-6) and np.abs(v.sum(axis=0)).max() < 1e-6
    with pytest.raises(ValueError):
        ula(0, 1.0)


def test_utils_against_closed_forms():
    from differt2d_amd.utils import beamformed_power, channel_matrix, mimo_capacity, singular_values, ula

    rng = np.random.default_rng(5)
    nr, nt, shape = 3, 4, (2, 5)
    # a rank-one H = alpha * a_rx a_tx^H per cell: second singular value 0, capacity log2(1 + snr / nt * |H|_F^2)
    alpha = (rng.normal(size=shape) + 1j * rng.normal(size=shape)) * 0.3
    arx = np.exp(2j * np.pi * rng.random((nr,) + shape))
    atx = np.exp(2j * np.pi * rng.random((nt,) + shape))
    H = alpha[None, None] * arx[:, None] * atx.conj()[None, :]
    ar = ArrayResponse(H.real.astype(F), H.imag.astype(F), np.zeros(shape, F))
    h = channel_matrix(ar)
    assert h.dtype == np.complex64 and h.shape == (nr, nt) + shape and np.array_equal(h.real, ar.re) and np.array_equal(h.imag, ar.im)
    s = singular_values(ar)
    assert s.dtype == np.float64 and s.shape == (3,) + shape
    fro2 = (np.abs(h.astype(np.complex128)) ** 2).sum(axis=(0, 1))
    assert np.allclose(s[0] ** 2, fro2, rtol=1e-6) and (s[1] <= 1e-6 * s[0]).all() and (s[2] <= 1e-6 * s[0]).all()
    snr = 37.0
    cap = mimo_capacity(ar, snr)
    assert cap.dtype == np.float64 and cap.shape == shape and np.allclose(cap, np.log2(1 + snr / nt * fro2), rtol=1e-6)
    # matched steering vectors on a line-of-sight H give nr * nt * |a|^2 (with unit-modulus weights w = a: |a^H H a|^2 =
    # |alpha|^2 (nr nt)^2, i.e. nr * nt * |a|^2 once the weights are normalised to unit norm)
    cell = (1, 3)
    wr, wt = arx[(slice(None),) + cell] / np.sqrt(nr), atx[(slice(None),) + cell] / np.sqrt(nt)
    p = beamformed_power(ar, wr, wt)
    assert p.dtype == np.float64 and p.shape == shape
    assert np.isclose(p[cell], nr * nt * np.abs(alpha[cell]) ** 2, rtol=1e-5)
    assert (p <= nr * nt * np.abs(alpha) ** 2 * (1 + 1e-5)).all()  # no other weights of unit norm do better (Cauchy-Schwarz)
    # the same through plane-wave phases: a line of sight seen along u, half-wavelength ULAs, weights matched to u
    u_t, u_r = np.array([np.cos(0.7), np.sin(0.7)]), np.array([np.cos(2.1), np.sin(2.1)])
    et, er = ula(nt, WL / 2).astype(np.float64), ula(nr, WL / 2, 0.4).astype(np.float64)
    a = 0.02
    Hl = a * np.exp(2j * np.pi * ((er @ u_r)[:, None] + (et @ u_t)[None, :]) / WL)
    one = ArrayResponse(Hl.real.astype(F)[..., None, None], Hl.imag.astype(F)[..., None, None], np.zeros((1, 1), F))
    w_r, w_t = np.exp(2j * np.pi * (er @ u_r) / WL) / np.sqrt(nr), np.exp(-2j * np.pi * (et @ u_t) / WL) / np.sqrt(nt)
    assert np.isclose(beamformed_power(one, w_r, w_t)[0, 0], nr * nt * a * a, rtol=1e-5)
    assert np.isclose(singular_values(one)[0, 0, 0], np.sqrt(nr * nt) * a, rtol=1e-5)
    # an identity channel: nt equal singular values, capacity nt * log2(1 + snr / nt)
    eye = ArrayResponse(np.eye(4, dtype=F)[..., None, None], np.zeros((4, 4, 1, 1), F), np.zeros((1, 1), F))
    assert np.allclose(singular_values(eye)[:, 0, 0], 1) and np.isclose(mimo_capacity(eye, 8.0)[0, 0], 4 * np.log2(3.0))
    with pytest.raises(ValueError, match="weights"):
        beamformed_power(ar, np.ones(4), np.ones(4))
    # a non-finite cell is NaN, the others are not
    bad = ArrayResponse(ar.re.copy(), ar.im.copy(), ar.total)
    bad.re[0, 0, 0, 0] = np.nan
    assert np.isnan(singular_values(bad)[:, 0, 0]).all() and np.isnan(mimo_capacity(bad, 1.0)[0, 0]) and np.isfinite(mimo_capacity(bad, 1.0)[1, 1])


# ---- bindings --------------------------------------------------------------------------------------------------------------------------
def test_bindings_and_abi_version():
    from differt2d_amd import _lib as L
    from differt2d_amd import utils
    from differt2d_amd.engine import ArrayResponse as AR, Context
    from differt2d_amd.scene import Scene

    assert L.D2D_ABI_VERSION == 12 and L.D2D_ARRAY_MAX == ARRAY_MAX == 8
    names = [s[0] for s in L.SYMBOLS]
    assert "d2d_array_response_launch" in names and "d2d_get_array_response" in names and "d2d_selftest_steer" in names
    assert callable(Context.array_response) and callable(Context.launch_array_response) and callable(Context.get_array_response)
    assert callable(Context.selftest_steer)
    assert callable(Scene.array_response_on_receivers_grid) and callable(Scene.array_response_on_transmitters_grid)
    assert AR._fields == ArrayResponse._fields == ("re", "im", "total")
    assert all(callable(getattr(utils, n)) for n in ("ula", "channel_matrix", "beamformed_power", "singular_values", "mimo_capacity"))
    header = open(os.path.join(ROOT, "include", "d2d.h")).read()
    assert "#define D2D_ARRAY_MAX 8" in header and "#define D2D_ABI_VERSION 12" in header
    assert "int d2d_array_response_launch(" in header and "int d2d_get_array_response(" in header


def test_scene_refuses_a_fun_that_is_not_fused_and_names_the_sparse_route():
    from differt2d_amd import _lib as L
    from differt2d_amd.scene import Scene
    from differt2d_amd.utils import ula

    scene = Scene.square_scene_with_obstacle()
    X, Y = unit_grid(4, 3)

    def step(tx, rx, path, objs):
        return (path.length() < 1.0).astype(F)

    for method in (scene.array_response_on_receivers_grid, scene.array_response_on_transmitters_grid):
        with pytest.raises(L.D2DUnsupported, match="valid_paths") as e:
            next(iter(method(X, Y, step, wavelength=WL, tx_elements=ula(2, WL / 2), rx_elements=ula(2, WL / 2))))
        assert "trace_paths" in str(e.value)
