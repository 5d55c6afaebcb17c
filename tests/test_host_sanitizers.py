"""CPU sanitizer runs (never on the GPU: the pool has no GPU ASan).

* the C oracle's sanitizer build (`make -C oracle asan`: -fsanitize=address,undefined) sweeps small and degenerate inputs;
* the host-only logic of libd2d.so -- differt2d_amd/csrc/d2d_host.hpp: candidate enumeration, parameter validation, the
  sweep thresholds, the LDS / heavy-list size arithmetic with its 4 GiB guard, the reverse sweep's trajectory chunks -- compiled with g++ -fsanitize=address,undefined
  (tests/native/d2d_host_san.cpp) and driven through ctypes with edge cases;
* the owning types of the context's GPU resources -- differt2d_amd/csrc/d2d_own.hpp -- in the same library, over a counting
  stand-in for the runtime: every allocation freed exactly once through growth, moves, rotation and partial construction.

Both run in a child process with libasan preloaded (an instrumented library cannot be loaded into a plain python
otherwise); any sanitizer report makes the child exit non-zero.
"""

import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _libasan():
    out = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return out if os.path.isabs(out) and os.path.exists(out) else None


def _run_child(code, preload):
    env = dict(os.environ, LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-c", textwrap.dedent(code)], capture_output=True, text=True, env=env, timeout=600)


@pytest.fixture(scope="module")
def asan():
    lib = _libasan()
    if lib is None:
        pytest.skip("gcc's libasan.so is not available")
    return lib


def test_oracle_under_asan_and_ubsan(asan):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "asan"])
    code = f"""
        import ctypes as C, sys
        import numpy as np
        sys.path.insert(0, {ROOT!r})
        from oracle import c_oracle as CO
        CO._LIB_PATH = {os.path.join(ROOT, "oracle", "libd2d_oracle_asan.so")!r}
        CO._lib = None
        rng = np.random.default_rng(0)
        F = np.float32
        cases = 0
        for n in (0, 1, 2, 5, 9):
            walls = rng.random((n, 2, 2), dtype=F)
            if n >= 2:
                walls[1] = walls[0]                      # two identical walls
                walls[0, 1] = walls[0, 0]                # a zero-length wall
            tx = rng.random(2, dtype=F)
            for shape in ((1, 1), (3, 5), (8, 8)):
                X, Y = rng.random(shape, dtype=F), rng.random(shape, dtype=F)
                X[0, 0], Y[0, 0] = tx                    # a cell on the transmitter
                for kw in (dict(approx=False), dict(approx=True), dict(approx=True, function="sigmoid", alpha=10.0)):
                    for lo, hi in ((0, 0), (0, 2), (3, 3) if n <= 5 else (1, 2)):
                        for role in ("rx", "tx"):
                            for prune in (False, True):
                                allowed = None if n < 3 else (np.arange(n) % 3 != 1).astype(np.uint8)
                                out, cnt = CO.power_and_count_maps(walls, tx, X, Y, allowed=allowed, min_order=lo, max_order=hi,
                                                                   prune=prune, grid_role=role, patch=0.01, **kw)
                                assert out.shape == shape and cnt.shape == shape
                                cases += 1
            if n:
                v, f, idx = CO.eval_candidates(walls, tx, tx + F(0.1), min_order=0, max_order=2)
                assert len(v) == CO.num_candidates(n, 0, 2)
        print("ORACLE-SAN-OK", cases)
    """
    out = _run_child(code, asan)
    assert out.returncode == 0 and "ORACLE-SAN-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-6000:]


def _build_host_san(tmp_path):
    so = str(tmp_path / "libd2d_host_san.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-shared", "-fPIC", "-Wall", "-Wextra", "-o", so, os.path.join(ROOT, "tests", "native", "d2d_host_san.cpp")])
    return so


def test_libd2d_host_logic_under_asan_and_ubsan(asan, tmp_path):
    so = _build_host_san(tmp_path)
    code = f"""
        import ctypes as C, itertools, sys
        import numpy as np
        sys.path.insert(0, {ROOT!r})
        from differt2d_amd._lib import Params
        L = C.CDLL({so!r})
        i64 = C.c_int64
        L.san_count.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(i64)]
        L.san_enumerate.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, i64]
        L.san_check_params.argtypes = [C.POINTER(Params), C.c_char_p, C.c_int]
        L.san_integer_pow.restype = C.c_float
        L.san_integer_pow.argtypes = [C.c_float, C.c_int]
        L.san_lds.argtypes = [C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_uint64)] * 3
        L.san_heavy_plan.argtypes = [C.c_longlong] * 4 + [C.POINTER(C.c_longlong)]

        def python_enum(n, allowed, lo, hi):
            ok = [j for j in range(n) if allowed is None or allowed[j]]
            out = []
            for k in range(lo, hi + 1):
                out += [t for t in itertools.product(ok, repeat=k) if all(a != b for a, b in zip(t, t[1:]))]
            return out

        # ---- enumeration: exact capacity (one element less must be refused, not overrun), filters, every order
        for n in (0, 1, 2, 3, 7):
            for allowed in (None, np.array([j % 2 == 0 for j in range(n)], np.uint8), np.zeros(n, np.uint8)):
                ap = None if allowed is None else allowed.ctypes.data_as(C.c_void_p)
                for lo, hi in ((0, 0), (0, 1), (0, 2), (2, 2), (0, 4), (3, 4), (2, 1)):
                    want = python_enum(n, allowed, lo, hi)
                    cnt = i64(-1)
                    assert L.san_count(n, ap, lo, hi, C.byref(cnt)) == 0 and cnt.value == len(want), (n, lo, hi, cnt.value, len(want))
                    cand = np.full((max(len(want), 1), 4), 99, np.int32)   # EXACTLY count rows: an overrun is an ASan report
                    order = np.full(max(len(want), 1), 99, np.int32)
                    rc = L.san_enumerate(n, ap, lo, hi, cand.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p), len(want))
                    assert rc == 0
                    got = [tuple(int(v) for v in cand[i, : order[i]]) for i in range(len(want))]
                    assert got == want
                    assert all((cand[i, order[i]:] == -1).all() for i in range(len(want)))
                    if len(want) > 0:
                        assert L.san_enumerate(n, ap, lo, hi, cand.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p), len(want) - 1) == -1
                    assert L.san_enumerate(n, ap, lo, hi, None, None, len(want)) == 0      # both outputs optional
        cnt = i64(0)
        assert L.san_enumerate(3, None, 0, 5, None, None, 10**9) == -1                   # order above D2D_MAX_ORDER
        assert L.san_enumerate(3, None, -1, 2, None, None, 10**9) == -1
        assert L.san_count(-1, None, 0, 1, C.byref(cnt)) == -1 and L.san_count(3, None, 0, 1, None) == -1
        assert L.san_count(2**31 - 1, None, 0, 2, C.byref(cnt)) == 0 and cnt.value == 1 + (2**31 - 1) + (2**31 - 1) * (2**31 - 2)
        assert L.san_count(2**31 - 1, None, 0, 4, C.byref(cnt)) == -1          # 2^124 candidates: refused, no signed overflow
        # ---- parameter validation
        def params(**kw):
            p = Params(min_order=0, max_order=2, approx=0, act=0, alpha=100.0, tol=1e-2, patch=0.0, seg_tol=0.005, fun_id=0,
                       r_coef=0.5, height=0.1, solver=0, steps=100, out_mode=0, grid_role=0, strict_nan=0, many=1)
            for k, v in kw.items():
                setattr(p, k, v)
            return p
        msg = C.create_string_buffer(8)   # tiny buffer: the message must be truncated, not overrun
        assert L.san_check_params(C.byref(params()), msg, 8) == 0
        for bad, rc in ((dict(min_order=-1), -1), (dict(max_order=5), -1), (dict(approx=1, alpha=0.0), -1), (dict(approx=1, alpha=float("nan")), -1),
                        (dict(approx=1, act=7), -4), (dict(fun_id=9), -4), (dict(fun_id=-1), -4), (dict(out_mode=2), -1), (dict(grid_role=-3), -1),
                        (dict(seg_tol=-0.1), -1), (dict(seg_tol=float("nan")), -1)):
            assert L.san_check_params(C.byref(params(**bad)), msg, 8) == rc, bad
            assert len(msg.value) <= 7
        assert L.san_check_params(None, msg, 8) == -1
        assert L.san_check_params(C.byref(params(max_order=5)), None, 0) == -1
        # ---- lax.integer_pow
        for x in (0.5, -1.25, 0.0, 3.0):
            ref = np.float32(1.0)
            for n in range(0, 9):
                got = L.san_integer_pow(x, n)
                assert got == np.float32(x) ** n or abs(got - float(np.float32(x)) ** n) <= 1e-6 * abs(got), (x, n, got)
        # ---- content hash of a grid (d2d_set_grid): every length incl. odd tails read exactly (ASan), any single bit matters
        L.san_hash_floats.restype = C.c_uint64
        L.san_hash_floats.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
        rng = np.random.default_rng(0)
        seen = set()
        for n in (0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000, 4099):
            a = rng.random(n, dtype=np.float32)   # EXACTLY n floats: reading past the end is an ASan report
            h = L.san_hash_floats(a.ctypes.data_as(C.c_void_p), n, 5)
            assert h == L.san_hash_floats(a.copy().ctypes.data_as(C.c_void_p), n, 5) and h not in seen
            seen.add(h)
            assert n == 0 or L.san_hash_floats(a.ctypes.data_as(C.c_void_p), n, 6) != h
            for i in ([0, n // 2, n - 1] if n else []):
                b = a.copy()
                b.view(np.uint32)[i] ^= np.uint32(1 << int(rng.integers(0, 32)))
                assert L.san_hash_floats(b.ctypes.data_as(C.c_void_p), n, 5) != h, (n, i)
            if n >= 2:
                b = a.copy(); b[0], b[1] = a[1], a[0]
                assert (a[0] == a[1]) or L.san_hash_floats(b.ctypes.data_as(C.c_void_p), n, 5) != h
        z, nz = np.zeros(4, np.float32), np.array([0.0, -0.0, 0.0, 0.0], np.float32)
        assert L.san_hash_floats(z.ctypes.data_as(C.c_void_p), 4, 0) != L.san_hash_floats(nz.ctypes.data_as(C.c_void_p), 4, 0)  # bit patterns
        # ---- LDS sizes: monotone, aligned, inside each other
        prev = 0
        for n in (0, 1, 50, 200, 1023, 1024, 5000):
            t, b, tot = C.c_uint64(), C.c_uint64(), C.c_uint64()
            L.san_lds(n, 4, 16, C.byref(t), C.byref(b), C.byref(tot))
            assert t.value == (4 * n + 1) * 16 + 512 and t.value > prev
            assert b.value % 16 == 0 and b.value >= t.value - 512 + 3 * 16 * 64 * 4 and tot.value == b.value + 4 * 512
            prev = t.value
        # ---- heavy-list plan: sizes consistent; the 4 GiB guard switches the cut off instead of overflowing
        out = (C.c_longlong * 4)()
        for tiles, Nc, hs, parts in ((16384, 50, 64, 4), (100, 50, 64, 4), (15, 50, 64, 4), (16384, 1, 64, 4), (16384, 50, 0, 4),
                                      (2**31 - 1, 256, 2**40, 4), (2**31 - 1, 2**20, 2**40, 4), (2**62, 2**31, 2**62, 4),
                                      (16384, 50, 64, 0), (-5, 50, 64, 4)):
            L.san_heavy_plan(tiles, Nc, hs, parts, out)
            H, cap, lf, ci = out[0], out[1], out[2], out[3]
            if H == 0:
                assert (cap, lf, ci) == (0, 0, 0)
                continue
            assert H == min(hs, tiles // 4, ((4 << 30) // 256) // (parts * cap)) and cap >= (Nc // parts + 1) * (Nc - 1) + Nc + 1   # covers a part's candidates
            assert lf == H * parts * cap * 64 and ci == H * parts * 65 and lf * 4 <= 4 << 30
        L.san_heavy_plan(16384, 50, 64, 4, out)
        assert out[0] == 64 and out[1] == -(-50 * 49 // 3) + 52       # the benchmark's own launch (parts by rank: a third each at most)
        L.san_heavy_plan(2**31 - 1, 256, 2**40, 4, out)
        assert 0 < out[0] == ((4 << 30) // 256) // (4 * out[1]) and out[2] * 4 <= 4 << 30   # as many as fit below 4 GiB
        # ---- region-list plan: every list owns a chunk, the levels nest, absurd sizes switch the lists off
        L.san_region_plan.argtypes = [C.c_int, C.c_int, C.c_longlong] + [C.c_int] * 5 + [C.c_longlong, C.c_int, C.POINTER(C.c_longlong)]
        L.san_region_plan.restype = None
        o = (C.c_longlong * 12)()
        for tx_, ty_, Nc, lo, hi, Rl, Rt, S, budget in ((128, 128, 50, 0, 2, 4, 16, 0, 512 << 20), (256, 256, 200, 0, 3, 4, 16, 0, 512 << 20),
                                                      (1, 1, 2, 2, 2, 4, 16, 0, 1 << 20), (128, 128, 50, 3, 4, 4, 6, 7, 512 << 20),
                                                      (128, 128, 1, 0, 2, 4, 16, 0, 512 << 20), (128, 128, 50, 0, 1, 4, 16, 0, 512 << 20),
                                                      (2**31 - 1, 2**31 - 1, 50, 0, 2, 1, 1, 0, 2**62), (128, 128, 50, 0, 2, 4, 16, 0, 1024),
                                                      (128, 128, 2**40, 0, 4, 4, 16, 0, 2**40), (0, 5, 50, 0, 2, 4, 16, 0, 1 << 30),
                                                      (128, 128, 50, 0, 2, 0, 16, 0, 1 << 30), (128, 128, 50, 0, 2, 4, 16, 5000, 1 << 30)):
            L.san_region_plan(tx_, ty_, Nc, lo, hi, Rl, Rt, S, budget, 128, o)
            if not o[0]:
                continue
            tR, tS, tr, ts, lR, lS, lr, ls, nst, mc, klo = [o[i] for i in range(1, 12)]
            assert lR == Rl and lS == 1 and tR % lR == 0 and tR >= lR and 1 <= tS <= 1024
            assert lr == -(-tx_ // lR) * -(-ty_ // lR) == ls and tr == -(-tx_ // tR) * -(-ty_ // tR) and ts == tr * tS
            assert klo == max(2, lo) <= hi and nst == (ls + ts) * (hi - klo + 1) and 2 * nst <= mc <= 2**31 - 1 and mc * 128 * 8 <= budget
        L.san_region_plan(128, 128, 50, 0, 2, 4, 16, 0, 512 << 20, 128, o)
        assert list(o) == [1, 16, 13, 64, 832, 4, 1, 1024, 1024, 1856, 524288, 2]   # the benchmark's own launch
        L.san_region_plan(128, 128, 50, 0, 1, 4, 16, 0, 512 << 20, 128, o)
        assert o[0] == 0                                                            # orders <= 1: no lists
        L.san_region_plan(2**31 - 1, 2**31 - 1, 50, 0, 2, 1, 1, 0, 2**62, 128, o)
        assert o[0] == 0                                                            # 2^62 regions: refused
        # ---- scalar thresholds of a sweep (sweep_thresholds): edge inputs, then values recorded from the inline code it replaced
        L.san_sweep_thresholds.argtypes = [C.POINTER(Params), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.san_sweep_thresholds.restype = None
        def thresholds(p, grad):
            d, f, i = np.zeros(3, np.float64), np.zeros(12, np.float32), np.zeros(3, np.int32)   # EXACTLY as many as it writes
            L.san_sweep_thresholds(C.byref(p), grad, d.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p))
            return d, f, i
        n_thr = 0
        for approx, act in ((0, 0), (1, 0), (1, 1)):                      # hard, hard_sigmoid, sigmoid
            for tol in (0.0, 1e-38, 0.5, 1.0):
                for alpha in (1e-30, 1e-6, 100.0, 1e6, 3e38):
                    for r_coef, height in ((0.5, 0.1), (-0.5, 0.1), (-3.0, 0.0), (0.5, 0.0)):
                        for fun_id in range(5):
                            for grad in (0, 1):
                                p = params(approx=approx, act=act, tol=tol, alpha=alpha, r_coef=r_coef, height=height, fun_id=fun_id)
                                d, f, i = thresholds(p, grad)
                                mode = 0 if not approx else (1 if act == 0 else 2)
                                assert i[0] == mode and f[7] == 1.0 and f[8] == np.float32(r_coef) and f[5] == np.float32(height) * np.float32(height)
                                assert (d[0] == 0.0) == (not approx) and d[1] <= d[0] * (1 + 1e-5)
                                assert d[2] == (17.5 / np.float64(np.float32(alpha)) if (mode == 2 and not grad) else d[0])
                                assert not (f[0] > f[1]) and not (f[2] > f[3])
                                assert (f[4] == -1.0) == (not np.float32(tol) > np.float32(1e-30))
                                assert fun_id != 4 or i[1] == 0
                                assert approx or i[2] == (np.float32(tol) <= 0.5)
                                n_thr += 1
        assert n_thr == 3 * 4 * 5 * 4 * 5 * 2
        recorded = [
            (dict(approx=0, act=0, alpha=100, tol=0.00999999978, seg_tol=0.00499999989, r_coef=0.5, height=0.100000001, fun_id=0, min_order=0, max_order=2), 0,
             [0x0000000000000000, 0x0000000000000000, 0x0000000000000000],
             [0xbba3d775, 0x3f80a42b, 0x8da24260, 0x3f800054, 0x3c23ad19, 0x3c23d70b, 0x40d4a2a9, 0x3f800000, 0x3f000000, 0x3e800000, 0x3e000000, 0x3d800000],
             [0, 1, 1]),
            (dict(approx=1, act=0, alpha=100, tol=0.5, seg_tol=0.00499999989, r_coef=-0.5, height=0.100000001, fun_id=0, min_order=0, max_order=2), 1,
             [0x3f9eb851eb851eb8, 0x3f9eb8660d7b12c6, 0x3f9eb851eb851eb8],
             [0xbd0f5c87, 0x3f847b38, 0xbcf5c330, 0x3f83d761, 0x327ae148, 0x3c23d70b, 0x40d4a2a9, 0x3f800000, 0xbf000000, 0x3e800000, 0xbe000000, 0x3d800000],
             [1, 0, 1]),
            (dict(approx=1, act=1, alpha=10, tol=0.5, seg_tol=0, r_coef=0.5, height=1, fun_id=0, min_order=0, max_order=3), 0,
             [0x4021cccccccccccd, 0x3ffc0012599ed7c8, 0x3ffc000000000000],
             [0xbfe00093, 0x40300073, 0xc10e66c4, 0x411e66ce, 0x327ae148, 0x3f800000, 0x3a83126f, 0x3f800000, 0x3f000000, 0x3e800000, 0x3e000000, 0x3d800000],
             [2, 1, 0]),
            (dict(approx=1, act=1, alpha=1000000, tol=1, seg_tol=0.00499999989, r_coef=0.5, height=0.100000001, fun_id=3, min_order=1, max_order=4), 0,
             [0x3f1754b05b7cfe58, 0x3ef259aade68eb21, 0x3ef2599ed7c6fbd2],
             [0xbba46a43, 0x3f80a4be, 0xb8baa5fd, 0x3f80033e, 0x32fae148, 0x3c23d70b, 0x00000000, 0x3f800000, 0x3f000000, 0x3e800000, 0x3e000000, 0x3d800000],
             [2, 1, 0]),
            (dict(approx=1, act=1, alpha=9.99999997e-07, tol=0, seg_tol=0.00499999989, r_coef=-3, height=0, fun_id=1, min_order=0, max_order=2), 1,
             [0x4195382100e618a6, 0x4170b080f0b4f9f7, 0x4195382100e618a6],
             [0xcca9c177, 0x4ca9c177, 0xcca9c177, 0x4ca9c177, 0xbf800000, 0x00000000, 0x7149f2ca, 0x3f800000, 0xc0400000, 0x41100000, 0xc1d80000, 0x42a20000],
             [2, 1, 0]),
            (dict(approx=0, act=1, alpha=100, tol=9.99999935e-39, seg_tol=0, r_coef=-0.5, height=0, fun_id=4, min_order=1, max_order=4), 1,
             [0x0000000000000000, 0x0000000000000000, 0x0000000000000000],
             [0x8da24260, 0x3f800054, 0x8da24260, 0x3f800054, 0xbf800000, 0x00000000, 0x7149f2ca, 0x3f800000, 0xbf000000, 0x3e800000, 0xbe000000, 0x3d800000],
             [0, 0, 1]),
        ]
        for kw, grad, want_d, want_f, want_i in recorded:
            d, f, i = thresholds(params(**kw), grad)
            assert d.view(np.uint64).tolist() == want_d and f.view(np.uint32).tolist() == want_f and i.tolist() == want_i, (kw, grad)
        # ---- cells per chunk of the reverse sweep's trajectory store (opt_chunk_cells): edge inputs, then recorded values
        L.san_opt_chunk_cells.argtypes = [C.c_longlong] * 3 + [C.c_int] + [C.c_longlong] * 2
        L.san_opt_chunk_cells.restype = C.c_longlong
        chunk = L.san_opt_chunk_cells
        for cells in (1, 10, 63, 64, 65, 810, 90000, 2**31 - 1):
            pad = -(-cells // 64) * 64
            for per_cell in (0, 1, 400, 123457, 2**40):
                for mb in (1, 7, 16384, 262144):
                    for known, free, resident in ((0, 0, 0), (1, 0, 0), (1, 1 << 20, 0), (1, 300 << 20, 4096), (1, 2**61, 2**61)):
                        n = chunk(cells, per_cell, mb, known, free, resident)
                        assert n % 64 == 0 and 64 <= n <= pad, (cells, per_cell, mb, known, free, resident, n)
                        budget = min(mb << 20, max((free + resident) // 2, 64 << 20)) if known else mb << 20
                        assert n == pad or n * 4 * max(per_cell, 1) <= budget or n == 64, (cells, per_cell, mb, n)
        assert chunk(10, 400, 1, 0, 0, 0) == 64 and chunk(10, 0, 1, 1, 0, 0) == 64                  # fewer than 64 cells: one wave
        assert chunk(90000, 2**40, 1, 0, 0, 0) == 64                                               # a budget below one wave: one wave
        assert chunk(90000, 400, 16384, 1, 0, 0) == 64 * ((64 << 20) // 1600 // 64)                # nothing free: the 64 MiB floor
        assert chunk(90000, 400, 16384, 1, 2**61, 2**61) == chunk(90000, 400, 16384, 0, 0, 0)      # plenty free: opt_traj_mb decides
        recorded = [   # (cells, floats per cell, opt_traj_mb, memory known, free bytes, resident bytes) -> the inline code's chunk
            (810, 0, 1, 0, 0, 0, 832), (810, 0, 16384, 1, 0, 0, 832), (810, 400, 1, 0, 0, 0, 640), (810, 400, 1, 1, 0, 0, 640),
            (810, 4000, 1, 0, 0, 0, 64), (810, 123457, 16384, 1, 0, 0, 128), (810, 123457, 16384, 1, 314572800, 4096, 256),
            (25600, 0, 1, 1, 0, 0, 25600), (25600, 4000, 16384, 1, 0, 0, 4160), (25600, 4000, 16384, 1, 314572800, 4096, 9792),
            (90000, 0, 1, 0, 0, 0, 90048), (90000, 400, 16384, 1, 0, 0, 41920), (90000, 123457, 16384, 0, 0, 0, 34752),
            (90000, 123457, 16384, 1, 268435456000, 1073741824, 34752), (1000000, 0, 1, 1, 0, 0, 262144),
            (1000000, 0, 16384, 0, 0, 0, 1000000), (1000000, 400, 16384, 1, 314572800, 4096, 98304),
        ]
        for *args, want in recorded:
            assert chunk(*args) == want, (args, want)
        print("HOST-SAN-OK")
    """
    out = _run_child(code, asan)
    assert out.returncode == 0 and "HOST-SAN-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-6000:]


def test_libd2d_ownership_under_asan_and_ubsan(asan, tmp_path):
    so = _build_host_san(tmp_path)
    code = f"""
        import ctypes as C
        L = C.CDLL({so!r})
        vp, ll = C.c_void_p, C.c_longlong
        for name, res, args in (("san_own_counts", None, [C.POINTER(ll)]), ("san_buf_new", vp, []), ("san_buf_delete", None, [vp]),
                                ("san_buf_ensure", C.c_int, [vp, C.c_uint64, C.c_int]), ("san_buf_release", None, [vp]),
                                ("san_buf_query", None, [vp, C.POINTER(ll)]), ("san_buf_move_construct", vp, [vp]),
                                ("san_buf_move_assign", None, [vp, vp]), ("san_ctx_new", vp, [C.c_int]), ("san_ctx_delete", None, [vp]),
                                ("san_ctx_rotate", None, [vp, C.c_int]), ("san_ctx_sets", None, [vp, C.POINTER(ll)])):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args

        def counts():
            o = (ll * 4)()
            L.san_own_counts(o)
            return dict(allocs=o[0], frees=o[1], bad=o[2], live=o[3])

        def query(b):    # (n, p set, bytes the stand-in was asked for)
            o = (ll * 3)()
            L.san_buf_query(b, o)
            return o[0], o[1], o[2]

        def balanced(live=0):
            c = counts()
            assert c["bad"] == 0 and c["allocs"] - c["frees"] == c["live"] == live, c
            return c

        # ---- ensure: grow / no-grow / zero; release, then ensure again
        b = L.san_buf_new()
        assert query(b) == (0, 0, -1) and balanced()["allocs"] == 0
        assert L.san_buf_ensure(b, 0, 0) == 0 and query(b) == (1, 1, 4)            # a count of 0 allocates 1
        assert L.san_buf_ensure(b, 1, 0) == 0 and balanced(1)["allocs"] == 1       # big enough: nothing happens
        assert L.san_buf_ensure(b, 100, 0) == 0 and query(b) == (100, 1, 400)      # grows by free-then-allocate
        assert balanced(1)["allocs"] == 2
        for count in (100, 7, 0):
            assert L.san_buf_ensure(b, count, 0) == 0 and query(b) == (100, 1, 400) and balanced(1)["allocs"] == 2
        assert L.san_buf_ensure(b, 101, 0) == 0 and query(b) == (101, 1, 404) and balanced(1)["allocs"] == 3
        L.san_buf_release(b)
        assert query(b) == (0, 0, -1) and balanced()["frees"] == 3
        L.san_buf_release(b)                                                       # twice: still one free per allocation
        assert balanced()["frees"] == 3
        assert L.san_buf_ensure(b, 5, 0) == 0 and query(b) == (5, 1, 20) and balanced(1)["allocs"] == 4
        # a failed growth reports the error, frees the old buffer and leaves the buffer empty and usable
        assert L.san_buf_ensure(b, 50, 1) == -2 and query(b) == (0, 0, -1) and balanced()["allocs"] == 4
        assert L.san_buf_ensure(b, 50, 0) == 0 and query(b) == (50, 1, 200) and balanced(1)
        # ---- move construction and move assignment, self-assignment included
        m = L.san_buf_move_construct(b)
        assert query(b) == (0, 0, -1) and query(m) == (50, 1, 200) and balanced(1)["allocs"] == 5
        L.san_buf_move_assign(m, m)                                                # self: untouched
        assert query(m) == (50, 1, 200) and balanced(1)
        assert L.san_buf_ensure(b, 3, 0) == 0 and balanced(2)
        L.san_buf_move_assign(b, m)                                                # the target's own buffer is freed
        assert query(b) == (50, 1, 200) and query(m) == (0, 0, -1) and balanced(1)
        L.san_buf_move_assign(b, m)                                                # from an empty one
        assert query(b) == (0, 0, -1) and query(m) == (0, 0, -1) and balanced()
        L.san_buf_move_assign(b, b)                                                # self, empty
        assert L.san_buf_ensure(m, 9, 0) == 0
        L.san_buf_delete(m)                                                        # the destructor frees
        L.san_buf_delete(b)
        assert balanced()["allocs"] == 7
        # ---- three PrepSet-like sets rotated the way take_prep_set rotates them: buffers, pointer, flags and event travel together
        base = counts()["allocs"]
        c = L.san_ctx_new(9)
        assert balanced(12)["allocs"] == base + 12    # 2 streams, 4 events, the pinned block, 2 + 3 buffers
        def sets():
            o = (ll * 15)()
            L.san_ctx_sets(c, o)
            return [tuple(o[5 * i: 5 * i + 5]) for i in range(3)]
        start = sets()
        assert start == [(100, 16, 1, 0, 1), (101, 17, 1, 1, 1), (102, 18, 1, 0, 1)]
        done = 0
        for times in (1, 1, 1, 2, 5, 300, 1001):
            L.san_ctx_rotate(c, times)
            done += times
            k = done % 3
            assert sets() == start[k:] + start[:k], (done, sets())   # cur <- spare[0] <- spare[1] <- cur
            assert counts()["bad"] == 0
        L.san_ctx_delete(c)
        balanced()
        # ---- destruction of a partly built aggregate (a d2d_create that fails at any step)
        for built in range(0, 10):
            c = L.san_ctx_new(built)
            L.san_ctx_delete(c)
            balanced()
        print("OWN-SAN-OK", counts())
    """
    out = _run_child(code, asan)
    assert out.returncode == 0 and "OWN-SAN-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-6000:]
