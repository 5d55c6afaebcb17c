"""Host side of the wideband array response (no GPU): the host's parameter and memory checks and its chunk plan through a plain g++
build of ``d2d_host.hpp`` (ctypes, and a stand-alone program, plain and with sanitizers), the oracle recipe of
``tests/array_frequency_response_oracle.py`` against the frequency response's (which the GPU tests then hold the kernel to),
``utils.channel_tensor`` / ``array_response_at`` / ``wideband_capacity`` against closed forms, and the bindings."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frequency_response_oracle as FRO
from array_frequency_response_oracle import ArrayFrequencyResponse, array_frequency_response, fold_list
from array_response_oracle import AMP_LINEAR, AMP_SQRT, unit_dir
from conftest import unit_grid
from test_gpu_power_angle import _directed
from test_gpu_strongest_paths import _case, _contributions

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "array_frequency_response_host.cpp")
GXX = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """d2d_host.hpp's wideband checks and chunk plan, compiled for the host (tests/native/array_frequency_response_host.cpp)."""
    so = str(tmp_path_factory.mktemp("afr_host") / "libafr_host.so")
    subprocess.check_call(GXX + ["-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.afr_params.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    lib.afr_params.restype = C.c_int
    lib.afr_bytes_per_cell.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.afr_bytes_per_cell.restype = C.c_longlong
    lib.afr_fits.argtypes = [C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong]
    lib.afr_fits.restype = C.c_int
    lib.afr_chunk_size.restype = C.c_int
    lib.afr_chunks.argtypes = [C.c_int]
    lib.afr_chunks.restype = C.c_int
    lib.afr_chunk.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 3
    lib.afr_chunk.restype = None
    return lib


def _params(host, inv, tx, rx, amp=0, nf=None, nt=None, nr=None):
    """``(status, index the message ends in or -1, message)``; a list given as None is handed over as NULL."""
    arr = [None if a is None else np.ascontiguousarray(a, F) for a in (inv, tx, rx)]
    ptr = [None if a is None else a.ctypes.data for a in arr]
    nf = arr[0].size if nf is None else nf
    nt = arr[1].size // 2 if nt is None else nt
    nr = arr[2].size // 2 if nr is None else nr
    at = C.c_int(0)
    msg = C.create_string_buffer(256)
    rc = host.afr_params(ptr[0], nf, amp, nt, ptr[1], nr, ptr[2], C.byref(at), msg, 256)
    return rc, at.value, msg.value.decode()


# ---- parameter checks ----------------------------------------------------------------------------------------------------------------
def test_wide_params_on_every_bad_count_and_names_the_bad_index(host):
    inv = np.array([20.0, 5.0, 0.0, 7.5, 12.0], F)
    tx, rx = np.full((4, 2), 0.025, F), np.zeros((3, 2), F)
    assert _params(host, inv, tx, rx, 0)[:2] == (0, -1) and _params(host, inv, tx, rx, 1)[:2] == (0, -1)
    assert _params(host, np.full(1024, 3.0, F), np.zeros((8, 2), F), np.zeros((8, 2), F))[:2] == (0, -1)
    # every bad count: the list of that count is not read (NULL)
    for bad in (0, -1, 1025, 2**30, -(2**30)):
        rc, at, msg = _params(host, None, tx, rx, nf=bad)
        assert (rc, at) == (-1, -1) and "nf in 1 .. 1024" in msg and msg.endswith(f"got {bad}")
    for bad in (0, -1, 9, 2**30, -(2**30)):
        rc, at, msg = _params(host, inv, None, None, nt=bad, nr=1)
        assert (rc, at) == (-1, -1) and "nt in 1 .. 8" in msg and msg.endswith(f"got {bad}")
        rc, at, msg = _params(host, inv, None, None, nt=1, nr=bad)
        assert (rc, at) == (-1, -1) and "nr in 1 .. 8" in msg and msg.endswith(f"got {bad}")
    # every position of the three lists, the index named
    for value in (np.nan, np.inf, -np.inf, -1.0, -1e-30):
        for k in range(inv.size):
            v = inv.copy()
            v[k] = value
            rc, at, msg = _params(host, v, tx, rx)
            assert (rc, at) == (-1, k) and "inv_wavelength" in msg and msg.endswith(f"at index {k}")
    for value in (np.nan, np.inf, -np.inf):
        for k in range(tx.size):
            e = tx.copy()
            e.reshape(-1)[k] = value
            rc, at, msg = _params(host, inv, e, rx)
            assert (rc, at) == (-1, k // 2) and "tx_elems" in msg
        for k in range(rx.size):
            e = rx.copy()
            e.reshape(-1)[k] = value
            rc, at, msg = _params(host, inv, tx, e)
            assert (rc, at) == (-1, k // 2) and "rx_elems" in msg
    for amp in (2, -1):
        rc, at, msg = _params(host, inv, tx, rx, amp)
        assert (rc, at) == (-1, -1) and "amplitude" in msg


def test_wide_fits_at_the_boundary_byte_and_with_sizes_that_would_wrap(host):
    assert [host.afr_bytes_per_cell(*p) for p in ((1, 1, 1), (9, 4, 3), (64, 4, 4), (1024, 8, 8))] == [12, 868, 8196, 524292]
    top = 2**64 - 1
    for mem_free in (0, 2**20, 3 * 2**30, 288 * 2**30, top):
        for held in (0, 2**16, 5 * 2**30, top):
            for nf, nt, nr in ((1, 1, 1), (9, 4, 3), (64, 4, 4), (1024, 8, 8)):
                per = 8 * nf * nt * nr + 4
                edge = (mem_free // 2 + held // 2) // per
                assert host.afr_fits(edge, nf, nt, nr, mem_free, held) == 1 and host.afr_fits(edge + 1, nf, nt, nr, mem_free, held) == 0
                # the boundary byte: one cell more fits exactly when the budget grows to hold it
                if mem_free == 288 * 2**30 and held == 0:
                    need = (edge + 1) * per  # bytes
                    assert host.afr_fits(edge + 1, nf, nt, nr, 2 * need, 0) == 1 and host.afr_fits(edge + 1, nf, nt, nr, 2 * need - 2, 0) == 0
    # 1024^2 cells, 64 wavelengths, 4 x 4: 8 GiB and 4 MiB of totals
    assert host.afr_fits(2**20, 64, 4, 4, 2 * 8196 * 2**20, 0) == 1 and host.afr_fits(2**20, 64, 4, 4, 2 * 8196 * 2**20 - 2, 0) == 0
    assert host.afr_fits(2**20, 1024, 8, 8, 288 * 2**30, 0) == 0  # (512 GiB: what no GPU test can hold)
    # cells * bytes per cell wraps 64 bits: still refused
    assert (top // 524292 + 2) * 524292 >= 2**64
    assert host.afr_fits(top // 524292 + 2, 1024, 8, 8, 288 * 2**30, 0) == 0 and host.afr_fits(top, 1024, 8, 8, 288 * 2**30, 0) == 0
    assert host.afr_fits(top // 12 + 2, 1, 1, 1, top, top) == 0 and host.afr_fits(2**62, 1, 1, 1, 2**40, 0) == 0
    # counts out of range never fit (and form no product)
    for bad in (0, -1, 2**30):
        assert host.afr_fits(1, bad, 1, 1, top, top) == 0 and host.afr_fits(1, 1, bad, 1, top, top) == 0 and host.afr_fits(1, 1, 1, bad, top, top) == 0


def test_chunks_cover_every_list_once_and_in_order(host):
    W = host.afr_chunk_size()
    assert W in (8, 16, 32, 64)
    first, count, with_total = C.c_int(), C.c_int(), C.c_int()
    for nf in range(1, 1025):
        n = host.afr_chunks(nf)
        assert n == -(-nf // W)
        covered = []
        for i in range(n):
            host.afr_chunk(nf, i, C.byref(first), C.byref(count), C.byref(with_total))
            assert 1 <= count.value <= W and with_total.value == (1 if i == 0 else 0), (nf, i)
            covered.extend(range(first.value, first.value + count.value))
        assert covered == list(range(nf)), nf


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_stand_alone_host_program(tmp_path, sanitize):
    """wide_params, wide_fits (refusals included) and the chunk plan in a program of their own; with sanitizers it is the same
    program, linked against the sanitizers' run times by the compiler (nothing is preloaded, nothing is loaded into Python)."""
    exe = str(tmp_path / "afr_host")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(GXX + extra + ["-DAFR_MAIN", "-o", exe, SRC])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(done.stdout)
    assert done.returncode == 0, done.stdout
    assert "array_frequency_response_host: 0 failures" in done.stdout


# ---- the oracle recipe ---------------------------------------------------------------------------------------------------------------
def _joined(scene, mode, role):
    _, T, Rl, _ = _contributions(scene, mode, role, "received_power")
    _, T2, D = _directed(scene, mode, role, "received_power")
    assert np.array_equal(T.view(np.uint32), T2.view(np.uint32))  # the two oracles' contributions agree in bits
    return T, Rl, D


INV_LIST = np.array([F(1) / F(0.05), 7.0, 0.0, 12.5], F)


@pytest.mark.parametrize("amp", [AMP_SQRT, AMP_LINEAR], ids=["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle", "square_centre"])
def test_zero_offset_pair_is_the_frequency_response_recipe_by_bits(scene, mode, role, amp):
    """A pair whose two offsets are (+-0, +-0) is the frequency response wherever no contribution lacks a direction: every cell of
    random7 and obstacle; in square_centre the line of sight of the cell that IS the fixed end point has none, and exactly [4, 4]
    differs."""
    T, Rl, D = _joined(scene, mode, role)
    etx = np.array([[0.0, -0.0], [0.03, 0.01]], F)
    erx = np.array([[0.02, -0.07], [-0.0, 0.0]], F)
    re, im, total = fold_list(T, Rl, D, INV_LIST, amp, etx, erx)
    fre, fim, ftotal = FRO.fold_list(T, Rl, INV_LIST, amp)
    assert re.shape == (4, 2, 2, T.shape[1]) and np.array_equal(_bits(total), _bits(ftotal))
    shape = _case(scene)[2].shape
    _, _, okt = unit_dir(D[:, :, 0], D[:, :, 1])
    _, _, okr = unit_dir(D[:, :, 2], D[:, :, 3])
    lacking = ((T != 0) & ~(okt & okr)).any(axis=0).reshape(shape)
    assert np.argwhere(lacking).tolist() == ([[4, 4]] if scene == "square_centre" else [])
    diff = (_bits(re[:, 1, 0]) != _bits(fre)) | (_bits(im[:, 1, 0]) != _bits(fim))
    for f in range(INV_LIST.size):
        assert np.argwhere(diff[f].reshape(shape)).tolist() == ([[4, 4]] if scene == "square_centre" else []), f
    assert np.count_nonzero(fim) > fim.size // 3
    # the planes off the origin are not the origin's, and the blocks differ from each other
    assert not np.array_equal(_bits(im[:, 0, 1]), _bits(fim)) and not np.array_equal(_bits(re[0]), _bits(re[1]))
    if amp == AMP_LINEAR:  # the entry 0: the fused map in re and +0.0 in im, except where the recipe leaves a contribution out
        keep = ~lacking.reshape(-1)
        assert np.array_equal(_bits(re[2, 1, 0])[keep], _bits(total)[keep]) and not _bits(im[2, 1, 0]).any()


def test_recipe_from_the_walls_on_a_grid_of_its_own():
    """array_frequency_response() end to end (what the GPU tests call for a grid they have no cached contributions of)."""
    from array_response_oracle import array_response

    walls, fixed, _, _ = _case("random7")
    X, Y = unit_grid(7, 5)
    kw = dict(min_order=0, max_order=2, approx=True, function="hard_sigmoid")
    etx, erx = np.array([[0.0, 0.0], [0.01, 0.03]], F), np.array([[-0.0, 0.0]], F)
    afr = array_frequency_response(walls, fixed, X, Y, INV_LIST[:3], AMP_SQRT, etx, erx, **kw)
    assert afr.re.shape == afr.im.shape == (3, 1, 2, 5, 7) and afr.total.shape == (5, 7)
    for f in range(3):
        ar = array_response(walls, fixed, X, Y, INV_LIST[f], AMP_SQRT, etx, erx, **kw)
        assert np.array_equal(_bits(afr.re[f]), _bits(ar.re)) and np.array_equal(_bits(afr.im[f]), _bits(ar.im))
        assert np.array_equal(_bits(afr.total), _bits(ar.total))
    assert afr.im[0].any() and not afr.im[2].any()


# ---- utils ---------------------------------------------------------------------------------------------------------------------------
def test_utils_against_closed_forms():
    from differt2d_amd.engine import ArrayResponse as AR
    from differt2d_amd.utils import array_response_at, channel_tensor, mimo_capacity, wideband_capacity

    rng = np.random.default_rng(11)
    nf, nr, nt, shape = 5, 3, 4, (2, 5)
    # a rank-one H = alpha * a_rx a_tx^H per wavelength and cell: capacity log2(1 + snr / nt * |H|_F^2) each, their mean over the band
    alpha = (rng.normal(size=(nf,) + shape) + 1j * rng.normal(size=(nf,) + shape)) * 0.3
    arx = np.exp(2j * np.pi * rng.random((nf, nr) + shape))
    atx = np.exp(2j * np.pi * rng.random((nf, nt) + shape))
    H = alpha[:, None, None] * arx[:, :, None] * atx.conj()[:, None, :]
    afr = ArrayFrequencyResponse(H.real.astype(F), H.imag.astype(F), rng.random(shape).astype(F))
    h = channel_tensor(afr)
    assert h.dtype == np.complex64 and h.shape == (nf, nr, nt) + shape and np.array_equal(h.real, afr.re) and np.array_equal(h.imag, afr.im)
    for f in (0, 3, -1):
        ar = array_response_at(afr, f)
        assert isinstance(ar, AR) and ar.re.shape == (nr, nt) + shape
        assert np.shares_memory(ar.re, afr.re) and np.shares_memory(ar.im, afr.im) and ar.total is afr.total  # views
        assert np.array_equal(ar.re, afr.re[f]) and np.array_equal(ar.im, afr.im[f])
    snr = 37.0
    fro2 = (np.abs(h.astype(np.complex128)) ** 2).sum(axis=(1, 2))  # [nf, m, n]
    cap = wideband_capacity(afr, snr)
    assert cap.dtype == np.float64 and cap.shape == shape
    assert np.allclose(cap, np.log2(1 + snr / nt * fro2).mean(axis=0), rtol=1e-6)
    assert np.allclose(cap, np.mean([mimo_capacity(array_response_at(afr, f), snr) for f in range(nf)], axis=0), rtol=1e-12)
    # one wavelength: mimo_capacity itself
    one = ArrayFrequencyResponse(afr.re[:1], afr.im[:1], afr.total)
    assert np.array_equal(wideband_capacity(one, snr), mimo_capacity(array_response_at(afr, 0), snr))
    # a NaN plane gives NaN in that cell only, an infinite one likewise
    for value in (np.nan, np.inf):
        bad = ArrayFrequencyResponse(afr.re.copy(), afr.im.copy(), afr.total)
        bad.im[3, 1, 2, 0, 4] = value
        got = wideband_capacity(bad, snr)
        assert np.isnan(got[0, 4]) and np.isnan(got).sum() == 1
        keep = np.ones(shape, bool)
        keep[0, 4] = False
        assert np.array_equal(got[keep], cap[keep])


# ---- bindings --------------------------------------------------------------------------------------------------------------------------
def test_bindings_and_abi_version():
    from differt2d_amd import _lib as L
    from differt2d_amd import utils
    from differt2d_amd.engine import ArrayFrequencyResponse as AFR, Context
    from differt2d_amd.scene import Scene

    assert L.D2D_ABI_VERSION == 12 and L.D2D_ARRAY_MAX == 8 and L.D2D_FREQ_MAX == 1024
    names = [s[0] for s in L.SYMBOLS]
    assert "d2d_array_frequency_response_launch" in names and "d2d_get_array_frequency_response" in names
    assert callable(Context.array_frequency_response) and callable(Context.launch_array_frequency_response)
    assert callable(Context.get_array_frequency_response)
    assert callable(Scene.array_frequency_response_on_receivers_grid) and callable(Scene.array_frequency_response_on_transmitters_grid)
    assert AFR._fields == ArrayFrequencyResponse._fields == ("re", "im", "total")
    assert all(callable(getattr(utils, n)) for n in ("channel_tensor", "array_response_at", "wideband_capacity"))
    header = open(os.path.join(ROOT, "include", "d2d.h")).read()
    assert "#define D2D_ABI_VERSION 12" in header
    assert "int d2d_array_frequency_response_launch(" in header and "int d2d_get_array_frequency_response(" in header
    lib = L.load()  # the library has both
    assert lib.d2d_array_frequency_response_launch and lib.d2d_get_array_frequency_response and lib.d2d_abi_version() == 12


def test_scene_refuses_a_fun_that_is_not_fused_and_names_both_routes():
    from differt2d_amd import _lib as L
    from differt2d_amd.scene import Scene
    from differt2d_amd.utils import ula

    scene = Scene.square_scene_with_obstacle()
    X, Y = unit_grid(4, 3)

    def step(tx, rx, path, objs):
        return (path.length() < 1.0).astype(F)

    e2 = ula(2, 0.025)
    for method in (scene.array_frequency_response_on_receivers_grid, scene.array_frequency_response_on_transmitters_grid):
        with pytest.raises(L.D2DUnsupported, match="valid_paths") as e:
            next(iter(method(X, Y, step, wavelengths=[0.05, 0.06], tx_elements=e2, rx_elements=e2)))
        assert "trace_paths" in str(e.value)
        # exactly one of the two wavelength arguments
        with pytest.raises(ValueError, match="exactly one"):
            method(X, Y, step, tx_elements=e2, rx_elements=e2)
        with pytest.raises(ValueError, match="exactly one"):
            method(X, Y, step, wavelengths=[0.05], inv_wavelengths=[20.0], tx_elements=e2, rx_elements=e2)
