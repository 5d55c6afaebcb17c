"""
GPU parity of the hand-derived value+grad kernel against reverse-mode autodiff of the oracle's op chain
(oracle/ref.py under torch.autograd, JAX-compatible where/min/max/logistic semantics).

Tolerance: BASELINE.json asks value+grad within 1e-5 fp32.  Values are bit-exact (hard, hard_sigmoid).
Gradients come out of a differently ordered fp32 backward pass, so they are compared against the fp64
autodiff result with atol = 3e-5 * max|grad| and rtol = 1e-4 (fp32 autodiff itself sits at ~3e-6 * max from
fp64).  NaN positions must coincide (the reference's `where`/sqrt(0) autodiff traps, mirrored on purpose).
"""

import glob
import os

import numpy as np
import pytest

from conftest import random_scene, unit_grid

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = sorted(p for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz"))
                if not os.path.basename(p).startswith("cfg"))  # cfg2_fullmap / cfg3_grad / cfg4_samples: full-size fixtures, own tests


@pytest.fixture(scope="module", params=["identity_order", "dearest_first"])
def ctx(request):
    from differt2d_amd.engine import Context

    with Context(0) as c:
        if request.param == "dearest_first":  # what grids of >= 2048 patches get (the schedule must not change the VJP)
            c.set_option("sched_min_tiles", 1)
        yield c


def _close(got, want, name):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, name
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), f"{name}: NaN positions differ ({nan_g.sum()} vs {nan_w.sum()})"
    if nan_w.all():
        return
    scale = np.nanmax(np.abs(want))
    err = np.nanmax(np.abs(got - want) - 1e-4 * np.abs(want))
    assert err <= 3e-5 * scale + 1e-6, f"{name}: max abs err {np.nanmax(np.abs(got - want)):.3e} at scale {scale:.3e}"


def _kwargs(d):
    kw = eval(str(d["kwargs"]))  # written by scripts/make_golden.py
    return kw


@pytest.mark.parametrize("strict_nan", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_against_golden_fixtures(ctx, path, strict_nan):
    """Both value+grad kernels: the default one (tile culling) and the exhaustive one (d2d_params.strict_nan)."""
    d = np.load(path)
    kw = dict(_kwargs(d), strict_nan=strict_nan)
    ctx.set_scene(d["walls"])
    got = ctx.value_and_grads(d["tx"], d["X"], d["Y"], **kw)
    if kw.get("function") == "sigmoid":
        np.testing.assert_allclose(got["value"], d["value"], rtol=2e-5, atol=1e-5)
    else:
        assert np.array_equal(got["value"], d["value"])
    _close(got["grad_rx"], d["grad_rx"], "grad_rx")
    _close(got["tx_bar"], d["tx_bar"], "tx_bar")
    _close(got["walls_bar"], d["walls_bar"], "walls_bar")
    # non-trivial cotangent
    got = ctx.value_and_grads(d["tx"], d["X"], d["Y"], cotangent=d["cot"], **kw)
    _close(got["tx_bar"], d["tx_bar_cot"], "tx_bar (cotangent)")
    _close(got["walls_bar"], d["walls_bar_cot"], "walls_bar (cotangent)")


@pytest.mark.parametrize("strict_nan", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("approx,function", [(False, "hard_sigmoid"), (True, "hard_sigmoid"), (True, "sigmoid")])
@pytest.mark.parametrize("fun", ["received_power", "length_squared", "length"])
def test_against_live_autodiff(ctx, approx, function, fun, strict_nan):
    from oracle import ref as R

    tx, walls = random_scene(10, seed=17)
    X, Y = unit_grid(19, 13)
    kw = dict(min_order=0, max_order=2, approx=approx, function=function, fun=fun)
    want = R.power_map_value_and_grads(walls, tx, X, Y, dtype="float64", **kw)
    ctx.set_scene(walls)
    got = ctx.value_and_grads(tx, X, Y, strict_nan=strict_nan, **kw)
    np.testing.assert_allclose(got["value"], want["value"], rtol=2e-5, atol=1e-5)
    for k in ("grad_rx", "tx_bar", "walls_bar"):
        _close(got[k], want[k], k)


def test_value_map_of_vg_kernel_is_bit_identical_to_forward(ctx):
    tx, walls = random_scene(20, seed=4)
    X, Y = unit_grid(64, 40)
    from differt2d_amd.engine import make_params

    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    for approx in (False, True):
        for strict in (False, True):
            p = make_params(max_order=2, approx=approx, strict_nan=strict)
            ctx.launch(p, tx)
            a = ctx.get_map()
            ctx.launch_vg(p, tx, scene_vjp=True)
            b = ctx.get_map()
            assert np.array_equal(a, b)


def test_los_gradients_analytic(ctx):
    # reference tests/test_scene.py:597-627: fun = length**2, no objects: grad = [2(X - tx_x), 2(Y - tx_y)]
    x = np.linspace(-3, 3, 10).astype(F)
    X, Y = np.meshgrid(x, x)
    ctx.set_scene(np.zeros((0, 2, 2), F))
    got = ctx.value_and_grads([1.0, 0.0], X, Y, max_order=1, fun="length_squared")
    want = np.stack([2 * (X - 1.0), 2 * Y], axis=-1)
    np.testing.assert_allclose(got["grad_rx"], want, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got["tx_bar"], -want.reshape(-1, 2).sum(0), rtol=1e-4, atol=1e-3)


def test_reduce_all_accumulates_gradients(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    tx, walls = random_scene(6, seed=8)
    tx2 = tx[::-1].copy()
    X, Y = unit_grid(16)
    ctx.set_scene(walls)
    a = ctx.value_and_grads(tx, X, Y, max_order=2, approx=True)
    b = ctx.value_and_grads(tx2, X, Y, max_order=2, approx=True)
    ctx.set_grid(X, Y)
    ctx.launch_vg(make_params(max_order=2, approx=True), tx, scene_vjp=True)
    ctx.launch_vg(make_params(max_order=2, approx=True, out_mode=L.OUT_ADD), tx2, scene_vjp=True)
    np.testing.assert_array_equal(ctx.get_map(), a["value"] + b["value"])
    np.testing.assert_array_equal(ctx.get_grad_rx(), a["grad_rx"] + b["grad_rx"])
    _, wb = ctx.get_scene_vjp()
    np.testing.assert_allclose(wb, a["walls_bar"] + b["walls_bar"], rtol=1e-5, atol=1e-4)


def test_culled_and_strict_gradients_agree_on_a_larger_grid(ctx):
    """cfg3-like: 50 walls, orders 0..2, 128 x 128 cells: the culled kernel drops 85 % of the candidates and must
    reproduce the exhaustive kernel's gradients (no NaN artefacts in this generic-position scene)."""
    tx, walls = random_scene(50, seed=1234)
    X, Y = unit_grid(128)
    ctx.set_scene(walls)
    for approx in (False, True):
        a = ctx.value_and_grads(tx, X, Y, max_order=2, approx=approx, strict_nan=False)
        b = ctx.value_and_grads(tx, X, Y, max_order=2, approx=approx, strict_nan=True)
        assert np.array_equal(a["value"], b["value"])
        assert np.array_equal(a["grad_rx"], b["grad_rx"], equal_nan=True)
        for k in ("tx_bar", "walls_bar"):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-6, atol=1e-6 * np.abs(b[k]).max())


def _same_flags_and_gradients(a, b, tag):
    assert np.array_equal(a["value"], b["value"], equal_nan=True), tag
    for k in ("grad_rx", "tx_bar", "walls_bar"):
        assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), f"{tag}: NaN positions of {k} differ"
    fin = ~np.isnan(b["grad_rx"])
    assert np.array_equal(a["grad_rx"][fin], b["grad_rx"][fin]), tag
    for k in ("tx_bar", "walls_bar"):
        f2 = ~np.isnan(b[k])
        if f2.any():
            np.testing.assert_allclose(a[k][f2], b[k][f2], rtol=1e-5, atol=1e-6 * float(np.abs(b[k][f2]).max()), err_msg=f"{tag}: {k}")


def test_nan_scan_with_a_full_queue_and_a_full_list():
    """The region scan's two bounded buffers -- the list of a round's survivors and the queue its probes are dealt through -- are
    sized so that they rarely fill; here they are made tiny ("nan_scan_wqcap" = 64 items instead of 2048, "nan_scan_rb" = 2
    batches = 128 list entries per round instead of 2048) so that a FULL queue and many rounds are the rule.  Round 5's queue took
    a reservation back when it was full and could then count slots nobody had written (the driver's GPU suite aborted in
    test_culled_and_strict_gradients_agree_on_a_larger_grid); the reservation is monotone now, every decoded item is
    checked before it addresses anything, and this test holds both: the counters say the queue overflowed (self_probes > 0), no
    item was ever refused (bad_items == 0), and the flags / gradients equal the exhaustive kernel's -- on the scene that aborted, on
    coarse and crowded ones (50 - 200 walls on 16^2 .. 128^2 cells: a region is a large part of the scene, nearly every candidate
    survives its box test), on lattice scenes where exact zeros are common, in both grid roles, launch after launch on one
    context (and after a small grid on the same context, the order of the suite that aborted)."""
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context

    rng = np.random.default_rng(2)
    with Context(0) as c:
        overflowed = nan_cells = 0
        # tiny buffers, degenerate ones (one queue slot, one batch per round), the product's sizes -- these three on the region
        # kernel's DEBUG instance (run-time sizes, counters: nan_scan_stats = 1) -- and the PRODUCT instance (compile-time sizes, no
        # counters: what every other launch of the library runs), whose queue overflows on the crowded scenes all the same
        for caps in ((64, 2, 1), (1, 1, 1), (0, 0, 1), (0, 0, 0)):
            c.set_option("nan_scan_wqcap", caps[0])
            c.set_option("nan_scan_rb", caps[1])
            c.set_option("nan_scan_stats", caps[2])
            # (a small grid first: the launch order of the suite that aborted)
            tx, walls = random_scene(10, seed=17)
            X, Y = unit_grid(19, 13)
            c.set_scene(walls)
            c.value_and_grads(tx, X, Y, max_order=2, approx=True)
            for nw, g, seed in ((50, 128, 1234), (50, 32, 1234), (120, 64, 7), (200, 16, 9)):
                tx, walls = random_scene(nw, seed=seed)
                X, Y = unit_grid(g)
                c.set_scene(walls)
                for role in (L.GRID_RX, L.GRID_TX):
                    for approx in (False, True):
                        if caps[:2] == (1, 1) and (nw > 50 or g > 32):
                            continue  # (one batch per round: thousands of barriers per region; the small case is enough)
                        kw = dict(min_order=0, max_order=2, approx=approx, grid_role=role)
                        b = c.value_and_grads(tx, X, Y, strict_nan=True, **kw)
                        for rep in range(3 if caps[0] else 1):
                            a = c.value_and_grads(tx, X, Y, strict_nan=False, **kw)
                            if caps[2]:
                                st = c.debug_nan_scan()
                                assert st["bad_items"] == 0, (caps, nw, g, role, approx, st)
                                if caps[0]:
                                    overflowed += int(st["self_probes"] > 0)
                            _same_flags_and_gradients(a, b, f"caps {caps}, {nw} walls, {g}^2, role {role}, approx {approx}, launch {rep}")
            # lattice scenes: exact zeros in the backward scan are common (NaN cells to find)
            for case in range(8):
                n = int(rng.integers(4, 12))
                walls = (np.round(rng.random((n, 2, 2)) * 4) / 4).astype(F)
                walls[(walls[:, 0] == walls[:, 1]).all(-1)] += F(0.125)
                tx = (np.round(rng.random(2) * 8) / 8).astype(F)
                xs = np.linspace(0, 1, int(rng.integers(17, 66))).astype(F)
                X, Y = np.meshgrid(xs, xs)
                c.set_scene(walls)
                kw = dict(min_order=0, max_order=2, approx=bool(case % 2), grid_role=L.GRID_TX if case % 4 >= 2 else L.GRID_RX)
                b = c.value_and_grads(tx, X, Y, strict_nan=True, **kw)
                a = c.value_and_grads(tx, X, Y, strict_nan=False, **kw)
                assert not caps[2] or c.debug_nan_scan()["bad_items"] == 0
                _same_flags_and_gradients(a, b, f"caps {caps}, lattice case {case}")
                nan_cells += int(np.isnan(b["grad_rx"]).any(-1).sum())
        print(f"launches with a full queue: {overflowed}; NaN cells compared on the lattice scenes: {nan_cells}")
        assert overflowed >= 40 and nan_cells > 100


def test_value_and_grad_in_a_scene_of_2000_walls(ctx):
    """The value+grad kernels with 128 KB of tables and adjoint tables in LDS (2 000 short walls; tests/test_gpu_forward.py has the
    forward sweep): orders 0..1 over all walls, both grid roles -- the culled sweep against the exhaustive kernel (values and
    per-cell gradients bit for bit, NaN positions included, scene VJP to rounding) and, on a block of cells, against the C gradient
    oracle."""
    from differt2d_amd import _lib as L
    from oracle import c_oracle as CO

    rng = np.random.default_rng(11)
    c = rng.random((2000, 2))
    ang = rng.random(2000) * np.pi
    d = np.stack([np.cos(ang), np.sin(ang)], -1) * 0.006
    tx, walls = np.array([0.4503, 0.5211], F), np.stack([c - d, c + d], 1).astype(F)
    X, Y = unit_grid(24, 16)
    X, Y = (X * F(0.3) + F(0.31)).astype(F), (Y * F(0.2) + F(0.42)).astype(F)
    ctx.set_scene(walls)
    for role, rname in ((L.GRID_RX, "rx"), (L.GRID_TX, "tx")):
        for approx in (False, True):
            kw = dict(min_order=0, max_order=1, approx=approx, grid_role=role)
            a = ctx.value_and_grads(tx, X, Y, strict_nan=False, **kw)
            b = ctx.value_and_grads(tx, X, Y, strict_nan=True, **kw)
            assert np.array_equal(a["value"], b["value"]) and np.count_nonzero(a["value"]) > 100
            assert np.array_equal(a["grad_rx"], b["grad_rx"], equal_nan=True)
            for k in ("tx_bar", "walls_bar"):
                assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k
                np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-6 * np.nanmax(np.abs(b[k])), err_msg=k)
            if (rname == "rx") != approx:  # (the oracle's dual numbers take seconds per 50 cells here: RX hard, TX hard_sigmoid, 8 x 6 cells)
                sub = (slice(5, 11), slice(8, 16))
                v, g = CO.power_map_grad(walls, tx, X[sub], Y[sub], min_order=0, max_order=1, approx=approx, grid_role=rname)
                assert np.array_equal(a["value"][sub], v)
                _close(a["grad_rx"][sub], g, f"2000 walls, {rname} grid, approx={approx}")


@pytest.mark.parametrize("approx", [False, True])
def test_cfg3_full_size_value_and_grad(ctx, approx):
    """BASELINE.json configs[2] at full size (50 walls, 1024 x 1024 cells, orders 0..2, value + grad): the value map of
    the reverse-mode sweep equals the forward sweep's bit for bit, and on a 32 x 32 block the per-cell gradients equal
    those of the exhaustive kernel run on that block alone."""
    tx, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(np.float32)
    X, Y = np.meshgrid(x, x)
    ctx.set_scene(walls)
    full = ctx.value_and_grads(tx, X, Y, max_order=2, approx=approx, strict_nan=False)
    assert np.array_equal(full["value"], ctx.power_map(tx, X, Y, max_order=2, approx=approx))
    i0, j0 = min(int(tx[1] * 1023), 1024 - 20) - 12, min(int(tx[0] * 1023), 1024 - 20) - 12
    sl = (slice(i0, i0 + 32), slice(j0, j0 + 32))  # around the transmitter: lit cells, non-zero gradients
    blk = ctx.value_and_grads(tx, X[sl], Y[sl], max_order=2, approx=approx, strict_nan=True)
    assert np.array_equal(full["value"][sl], blk["value"])
    fin = np.isfinite(blk["grad_rx"])
    assert fin.mean() > 0.99 and np.abs(blk["grad_rx"][fin]).max() > 0
    scale = np.abs(blk["grad_rx"][fin]).max()
    assert np.abs(full["grad_rx"][sl][fin] - blk["grad_rx"][fin]).max() <= 1e-6 * scale
    # The reference's autodiff NaN artefacts (un == 0 exactly, see DESIGN.md "NaN parity") do occur among 2.6e9
    # (cell, candidate) pairs: 35 cells in hard mode, 105 in hard_sigmoid mode, which -- as in the reference -- poison the
    # summed scene VJP (test_cfg3_full_map_nan_positions_equal_the_exhaustive_kernels holds every one of them to its place).
    nan_cells = np.isnan(full["grad_rx"]).any(-1)
    print("NaN cells:", int(nan_cells.sum()), "of", nan_cells.size)
    assert 0 < nan_cells.sum() < 1000


@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_cfg3_full_map_nan_positions_equal_the_exhaustive_kernels(role, mode):
    """"NaN positions must coincide".  The reference's reverse mode yields NaN wherever the backward
    scan of ANY candidate hits un == 0 (geometry.py:1105) or, in the approx modes, a zero-length segment (:227-228) -- valid
    candidate or not.  The default sweep (tile culling + the NaN scan, d2d_nanscan.hpp) against the exhaustive kernel
    (strict_nan: every candidate of every cell evaluated) on the WHOLE 1024 x 1024 map of configs[2], both grid roles:
    identical NaN positions in the per-cell gradient, in tx_bar and in walls_bar; identical values; equal finite gradients."""
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context

    kw = dict(approx=False) if mode == "hard" else dict(approx=True, function="hard_sigmoid")
    tx, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    kws = dict(min_order=0, max_order=2, grid_role=L.GRID_TX if role == "tx" else L.GRID_RX, **kw)
    with Context(0) as c:
        c.set_scene(walls)
        for _ in range(2):  # (the second launch runs on the work history, with the last-segment masks in use)
            a = c.value_and_grads(tx, X, Y, strict_nan=False, **kws)
        b = c.value_and_grads(tx, X, Y, strict_nan=True, **kws)
        c.set_option("nan_scan", 2)  # the scan's other shape (one wave per patch): the same flags
        a2 = c.value_and_grads(tx, X, Y, strict_nan=False, **kws)
    assert np.array_equal(a["value"], b["value"])
    n_nan = int(np.isnan(b["grad_rx"]).any(-1).sum())
    print(f"{role} {mode}: {n_nan} NaN cells, walls_bar NaN entries {int(np.isnan(b['walls_bar']).sum())}")
    assert n_nan >= 30, "the exhaustive kernel is expected to show the reference's NaN artefacts on this map"
    for got in (a, a2):
        for k in ("grad_rx", "tx_bar", "walls_bar"):
            assert np.array_equal(np.isnan(got[k]), np.isnan(b[k])), f"{k}: NaN positions differ"
        fin = ~np.isnan(b["grad_rx"])
        assert np.array_equal(got["grad_rx"][fin], b["grad_rx"][fin])
        for k in ("tx_bar", "walls_bar"):
            f2 = ~np.isnan(b[k])
            if f2.any():
                np.testing.assert_allclose(got[k][f2], b[k][f2], rtol=1e-6, atol=1e-6 * float(np.abs(b[k][f2]).max()))


@pytest.mark.parametrize("mode", ["hard", "hsig", "sigmoid"])
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_cfg3_rows_against_the_c_gradient_oracle(role, mode):
    """An independent checker at FULL size: every fourth row of configs[2] and the 64 rows around the fixed end point (311 296 cells; TX grids every eighth row;
    sigmoid, whose oracle costs 6x as much per row: 20 / 12 rows around the fixed end point) against oracle/d2d_oracle_grad.c -- forward-mode dual
    numbers through the C oracle's op chain, no adjoint code, nothing shared with the kernels (validated against reverse-mode
    autodiff of oracle/ref.py in tests/test_oracle_grad_c.py) -- computed live on the host cores.  The GPU runs its DEFAULT
    sweep (tile culling + NaN scan) over the whole grid.
    Values bit for bit (sigmoid: rtol 1e-6); NaN positions identical; every gradient entry within 1e-5 of the cell's gradient
    scale (sum over the candidates of |contribution gradient|: what an fp32 evaluation's rounding scales with) + 1e-5
    relative (sigmoid, which at alpha = 100 amplifies every rounding of its argument: 3e-4)."""
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context
    from oracle import c_oracle as CO

    kw = {"hard": dict(approx=False), "hsig": dict(approx=True, function="hard_sigmoid"),
          "sigmoid": dict(approx=True, function="sigmoid")}[mode]
    tx, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    i0 = min(max(int(tx[1] * 1023) - 32, 0), 1024 - 64)
    # Which rows: the oracle runs on the host's cores and the whole -m gpu suite has 900 s on the driver's box.  RX grids (the
    # benchmark's role): every fourth row + the 64 rows around the fixed end point; TX grids: every eighth + those 64 + the two rows
    # round 5's full-map run named; sigmoid: 20 rows (RX) / 12 rows (TX) around the fixed end point.  ALL 1 024 rows, both roles,
    # hard and hard_sigmoid: scripts/diag_rows.py <role> <mode> all (profiles/r06_parity_runs.txt).
    if mode == "sigmoid":
        rows = np.arange(i0 + 22, i0 + 42) if role == "rx" else np.arange(i0 + 26, i0 + 38)
    elif role == "rx":
        rows = np.unique(np.concatenate([np.arange(i0, i0 + 64), np.arange(0, 1024, 4)]))
    else:
        rows = np.unique(np.concatenate([np.arange(i0, i0 + 64), np.arange(0, 1024, 8), [197, 439]]))  # (197, 439: the tie cells of round 5's full-map run)
    at = int(np.searchsorted(rows, i0 + 31))  # two rows next to the fixed end point, by position in `rows`
    with Context(0) as c:
        c.set_scene(walls)
        got = c.value_and_grads(tx, X, Y, min_order=0, max_order=2, grid_role=L.GRID_TX if role == "tx" else L.GRID_RX, **kw)
    value, grad, gabs, tie = CO.power_map_grad(walls, tx, X[rows], Y[rows], min_order=0, max_order=2, prune=1, grid_role=role,
                                               with_gabs=True, with_kink=True, **kw)
    if mode == "sigmoid":
        np.testing.assert_allclose(got["value"][rows], value, rtol=1e-6, atol=1e-7)
    else:
        assert np.array_equal(got["value"][rows], value), "value map differs from the oracle's"
    g = got["grad_rx"][rows].astype(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(grad)), f"NaN positions differ: GPU {int(np.isnan(g).sum())}, oracle {int(np.isnan(grad).sum())}"
    fin = ~np.isnan(grad)
    err = np.abs(g - grad)
    # 1e-5 of the cell's own gradient scale + 1e-6 of the largest gradient in the cell's row
    rowscale = np.nanmax(np.abs(grad), axis=(1, 2), keepdims=True)
    rel = 3e-4 if mode == "sigmoid" else 1e-5
    bar = rel * gabs[..., None] + rel * np.abs(grad) + 1e-6 * rowscale
    worst = float(np.nanmax(np.where(fin, err / bar, 0.0)))
    # The checker must not share the kernels' shortcut.  `prune = 1` stops a candidate's occlusion fold at the
    # first occluder saturated to exactly 1 -- as the culled kernels do; the PLAIN oracle (prune = 0) follows every fold of every
    # candidate, JAX's tie rule included.  It runs (a) on whole rows spread over the map -- the two rows next to the fixed end
    # point, the rows round 5's full-map diagnostic named (TX hard_sigmoid: 197, 439) and a dozen more -- where the GPU is
    # compared with it DIRECTLY, and (b) on every cell of the full comparison that is beyond the bar.
    plain_rows = np.unique(np.concatenate([rows[at:at + 2], rows[np.isin(rows, [197, 439])],
                                           rows[np.linspace(0, rows.size - 1, 0 if mode == "sigmoid" else 5).astype(int)]]))
    sub = np.searchsorted(rows, plain_rows)
    v0, g0, kink = CO.power_map_grad(walls, tx, X[plain_rows], Y[plain_rows], min_order=0, max_order=2, prune=0,
                                     grid_role=role, with_kink=True, **kw)
    assert np.array_equal(v0, value[sub]) and np.array_equal(np.isnan(g0), np.isnan(grad[sub]))
    smooth = ~kink.astype(bool)[..., None].repeat(2, -1) & ~np.isnan(g0)  # (NaN cells: positions compared above, the bar is NaN there)
    assert not (np.abs(g0 - grad[sub]) > bar[sub])[smooth].any(), "the oracle's shortcut changes a gradient away from a tie"
    with np.errstate(invalid="ignore"):
        plain_over = np.argwhere(((np.abs(g0 - g[sub]) > bar[sub]) & ~np.isnan(g0)).any(-1))
    # ... on those rows the GPU may differ from the plain oracle beyond the bar only in a cell where the oracle itself met a tie of
    # a minimum / maximum between arguments of different derivative (the known deviation, DESIGN.md K2 "Ties": a candidate that
    # culling never evaluates, hidden by an occluder saturated to exactly 1, while another occluder sits exactly on a kink of relu6)
    not_tie = [(int(plain_rows[r_]), int(c_)) for r_, c_ in plain_over if not kink[r_, c_]]
    lit = gabs > 0
    # Cells of the FULL comparison beyond the plain bar (a handful in a million): each is given to the plain oracle on its own.
    #   * the GPU within the bar of the plain oracle: the shortcut was off, not the GPU;
    #   * else a tie cell of the plain oracle: the known deviation, counted and reported (cfg3: RX 3 cells, TX hard_sigmoid 2);
    #   * else the oracle's own conditioning: the oracle again with the cell and the fixed end point moved by ONE ulp either way --
    #     the GPU must sit within twice the largest change that makes to the oracle's gradient (a reflection point next to a wall's
    #     end: the activation's slope alpha / 6 multiplies every rounding of the point; no fp32 evaluation order is pinned tighter
    #     than its inputs);  anything else fails the test.
    over = np.argwhere((fin & (err > bar)).any(-1))
    assert len(over) <= 16, f"{len(over)} cells beyond the plain bar, worst {worst:.2f} x"
    n_tie_over = n_plain_ok = 0
    unexplained = []
    for r_, c_ in over:
        Xc, Yc = X[rows[r_]:rows[r_] + 1, c_:c_ + 1], Y[rows[r_]:rows[r_] + 1, c_:c_ + 1]
        _, gp, kp = CO.power_map_grad(walls, tx, Xc, Yc, min_order=0, max_order=2, prune=0, grid_role=role, with_kink=True, **kw)
        if (np.nan_to_num(np.abs(gp[0, 0] - g[r_, c_])) <= bar[r_, c_]).all():
            n_plain_ok += 1
            continue
        if kp[0, 0]:
            n_tie_over += 1
            continue
        sens = np.zeros(2)
        for dx, dy, dt in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            nudge = lambda a, d: np.nextafter(np.asarray(a, F), F(np.inf * d)) if d else np.asarray(a, F)  # noqa: E731
            _, g2 = CO.power_map_grad(walls, nudge(tx, dt), nudge(Xc, dx), nudge(Yc, dy), min_order=0, max_order=2, prune=0,
                                      grid_role=role, **kw)
            sens = np.maximum(sens, np.nan_to_num(np.abs(g2[0, 0] - gp[0, 0]), nan=np.inf))
        if (np.abs(gp[0, 0] - g[r_, c_]) > bar[r_, c_] + 2.0 * sens).any():
            unexplained.append((int(rows[r_]), int(c_), g[r_, c_].tolist(), gp[0, 0].tolist(), sens.tolist()))
    print(f"{role} {mode}: {rows.size} rows, {int(lit.sum())} cells with a path, {int(np.isnan(grad).any(-1).sum())} NaN cells, worst error / bar "
          f"{worst:.3f}; max |grad| {float(np.nanmax(np.abs(grad))):.3e}; plain oracle (prune = 0) on {plain_rows.size} whole rows: "
          f"{int(kink.sum())} tie cells of {kink.size}, {len(plain_over)} cells where the GPU is beyond the bar ({len(plain_over) - len(not_tie)} of them tie cells); "
          f"full comparison: {len(over)} cells beyond the bar -- {n_plain_ok} within the bar of the plain oracle, {n_tie_over} tie cells of the "
          f"plain oracle (the known deviation), {len(unexplained)} beyond the plain oracle's one-ulp sensitivity")
    assert not not_tie, f"GPU beyond the bar of the plain oracle away from any tie: {not_tie[:5]}"
    # (the known deviation, measured: scripts/plain_vs_pruned_oracle.py, profiles/r06_parity_runs.txt -- a fraction of a cell per row)
    assert n_tie_over <= 8 and len(plain_over) - len(not_tie) <= 4 * plain_rows.size
    assert lit.sum() > 10000
    assert not unexplained, unexplained[:5]


def test_tx_grid_culled_and_exhaustive_gradients_agree(ctx):
    """TX grids (the cells are transmitters, per-cell gradient w.r.t. the transmitter, scene.py:1617-1620): the culled
    value+grad kernel against the exhaustive one (strict_nan) on random scenes, all modes, orders up to 3 -- values bit
    for bit; gradients and scene VJP wherever the exhaustive kernel is finite."""
    from differt2d_amd import _lib as L

    rng = np.random.default_rng(17)
    for case in range(12):
        n = int(rng.integers(3, 22))
        rx, walls = random_scene(n, seed=100 + case)
        X, Y = unit_grid(int(rng.integers(9, 40)), int(rng.integers(9, 40)))
        mode = [dict(approx=False), dict(approx=True), dict(approx=True, function="sigmoid")][case % 3]
        kw = dict(min_order=0, max_order=3 if n <= 10 else 2, grid_role=L.GRID_TX, **mode)
        ctx.set_scene(walls)
        a = ctx.value_and_grads(rx, X, Y, strict_nan=False, **kw)
        b = ctx.value_and_grads(rx, X, Y, strict_nan=True, **kw)
        assert np.array_equal(a["value"], b["value"], equal_nan=True)
        for k in ("grad_rx", "tx_bar", "walls_bar"):
            assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), (case, k)
        fin = np.isfinite(b["grad_rx"])
        assert fin.mean() > 0.9
        scale = max(1e-30, float(np.abs(b["grad_rx"][fin]).max()))
        assert np.abs(a["grad_rx"][fin] - b["grad_rx"][fin]).max() <= 1e-5 * scale
        for k in ("tx_bar", "walls_bar"):
            f2 = np.isfinite(b[k])
            if f2.any():
                np.testing.assert_allclose(a[k][f2], b[k][f2], rtol=1e-5, atol=1e-5 * max(1e-30, float(np.abs(b[k][f2]).max())))


def test_lattice_scenes_against_the_c_gradient_oracle(ctx):
    """Walls snapped to a coarse lattice, a transmitter on a lattice point, cells on walls' lines: exact zeros in the backward
    scan are common.  Values, NaN positions and gradients of the default sweep and of the exhaustive kernel against
    oracle/d2d_oracle_grad.c, all modes and path functions (fun = 1 in hard mode: nothing is differentiated, no NaN), both roles."""
    from differt2d_amd import _lib as L
    from oracle import c_oracle as CO

    rng = np.random.default_rng(5)
    nan_seen = checked = 0
    for case in range(24):
        n = int(rng.integers(3, 9))
        walls = (np.round(rng.random((n, 2, 2)) * 4) / 4).astype(F)
        walls[(walls[:, 0] == walls[:, 1]).all(-1)] += F(0.125)
        tx = (np.round(rng.random(2) * 8) / 8).astype(F)
        xs = np.linspace(0, 1, int(rng.integers(9, 34))).astype(F)
        X, Y = np.meshgrid(xs, xs[: int(rng.integers(5, xs.size + 1))])
        approx, function = [(False, "hard_sigmoid"), (True, "hard_sigmoid"), (True, "sigmoid")][case % 3]
        fun = ["received_power", "one", "length", "length_squared"][(case // 3) % 4]
        role = "tx" if case % 2 else "rx"
        kw = dict(min_order=0, max_order=2, approx=approx, function=function, fun=fun, alpha=float(rng.choice([100.0, 16.0])))
        value, grad, gabs, kink = CO.power_map_grad(walls, tx, X, Y, grid_role=role, with_gabs=True, with_kink=True, **kw)
        stable = _stable_under_one_ulp(walls, tx, X, Y, value, grad, gabs, role, kw)
        ctx.set_scene(walls)
        for strict in (False, True):
            got = ctx.value_and_grads(tx, X, Y, strict_nan=strict, grid_role=L.GRID_TX if role == "tx" else L.GRID_RX, **kw)
            checked += _held_to_the_gradient_oracle(got, value, grad, gabs, kink, stable, function, (case, strict, kw, role))
        nan_seen += int(np.isnan(grad).any(-1).sum())
    assert nan_seen > 20 and checked > 2000


def _stable_under_one_ulp(walls, tx, X, Y, value, grad, gabs, role, kw):
    """Which cells have a gradient worth comparing -- decided by the oracle alone: its own result must survive a nudge of
    the fixed end point and of the cell by one ulp.  (A lattice scene puts end points ON walls' lines: the interaction
    points are then rounding noise, fp32 and fp64 autodiff of oracle/ref.py disagree in the first digit, and so do any
    two fp32 evaluation orders.)"""
    from oracle import c_oracle as CO

    up = lambda a: np.nextafter(np.asarray(a, F), F(np.inf))
    stable = np.ones(X.shape, bool)
    for tx2, X2, Y2 in ((up(tx), X, Y), (tx, up(X), up(Y))):
        v2, g2 = CO.power_map_grad(walls, tx2, X2, Y2, grid_role=role, **kw)
        with np.errstate(invalid="ignore"):
            stable &= np.abs(v2 - value) <= 1e-3 * np.abs(value) + 1e-9
            stable &= (np.abs(g2 - grad) <= 1e-2 * gabs[..., None] + 1e-9).all(-1)
    return stable


def _held_to_the_gradient_oracle(got, value, grad, gabs, kink, stable, function, tag):
    """The rule of ``test_lattice_scenes_against_the_c_gradient_oracle`` (tests/test_gpu_irregular_grids.py holds other grids to
    it): values by bits (sigmoid: rtol 1e-6, atol 1e-7), NaN positions identical, gradients within the bar below.  Returns the
    number of cells whose gradient was compared."""
    if function == "sigmoid":
        np.testing.assert_allclose(got["value"], value, rtol=1e-6, atol=1e-7)
    else:
        assert np.array_equal(got["value"], value, equal_nan=True), tag
    g = got["grad_rx"].astype(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(grad)), (tag, int(np.isnan(g).sum()), int(np.isnan(grad).sum()))
    # Gradients: wherever the oracle met no tie of a minimum / maximum between arguments with different tangents.
    # (At such a kink JAX returns the mean of the two one-sided derivatives; the image-method kernel sends the
    # cotangent to the first of the equal arguments -- DESIGN.md, "known deviations" -- and a lattice scene is
    # made of kinks.)  sigmoid at alpha = 100 amplifies every rounding of its argument: a wider bar there.
    fin = np.isfinite(grad).all(-1) & np.isfinite(g).all(-1) & ~kink & stable
    rel = 3e-4 if function == "sigmoid" else 1e-5
    bar = rel * gabs[..., None] + rel * np.abs(grad) + 1e-6
    bad = (np.abs(g - grad) > bar).any(-1) & fin
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:3].tolist())
    return int(fin.sum())


def _tight(got, want, want32, name, report):
    """north_star's bar: within 1e-5 (of the largest gradient, + 1e-5 relative) of the fp64 autodiff result; NaN positions
    identical.  Where the reference's OWN fp32 autodiff (same op chain, `want32`) is further than that from fp64 -- cells
    around the transmitter, where the gradient grows like 1/r^3 and every fp32 evaluation carries that round-off -- the
    bar is twice that cell's fp32-autodiff error: no fp32 evaluation can be held closer to fp64 than the reference is."""
    got, want, want32 = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(want32, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{name}: NaN positions differ"
    if not np.isfinite(want).any():
        return
    scale = float(np.nanmax(np.abs(want)))
    err = np.abs(got - want)
    ref_err = np.abs(want32 - want)
    plain = 1e-5 * scale + 1e-5 * np.abs(want) + 1e-7
    over_plain = np.nan_to_num(err) > plain
    report.append(f"{name}: max err/scale {float(np.nanmax(err)) / scale:.2e} (the reference's fp32 autodiff: "
                  f"{float(np.nanmax(ref_err)) / scale:.2e}); {int(over_plain.sum())} of {err.size} entries beyond 1e-5, "
                  f"every one of them within 2x the fp32-autodiff error at that entry")
    bad = np.nan_to_num(err) > np.maximum(plain, 2.0 * np.nan_to_num(ref_err) + 1e-7)
    assert not bad.any(), report[-1] + f" -- NOT so for {int(bad.sum())} entries, worst {float(np.nanmax(err[bad])):.3e}"


@pytest.mark.parametrize("strict_nan", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_cfg3_full_grid_blocks_against_autodiff_of_the_oracle(role, mode, strict_nan):
    """BASELINE.json configs[2] -- the 50-wall scene, 1024 x 1024 cells, orders 0..2, value + gradient -- against
    reverse-mode autodiff of the ORACLE (tests/golden/cfg3_grad_*.npz, scripts/make_golden_cfg3.py: oracle/ref.py under
    torch.autograd in fp64; NaN positions from the same chain in fp32) on 8 x 8 blocks of the full grid: the transmitter's
    patch and its neighbours, patches crossed by walls, random patches (768 cells as receivers, 256 as transmitters).
    The GPU sweeps the WHOLE grid (so every block is culled exactly as in the benchmark) for the values and the per-cell
    gradients, and the blocks alone for the scene VJP.  Tolerance: see _tight."""
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context

    z = np.load(os.path.join(os.path.dirname(__file__), "golden", f"cfg3_grad_{role}_{mode}.npz"))
    kw = dict(approx=False) if mode == "hard" else dict(approx=True, function="hard_sigmoid")
    tx, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    blocks = z["blocks"]
    ii = (blocks[:, 0, None, None] + np.arange(8)[None, :, None]) + np.zeros((1, 1, 8), np.int64)
    jj = (blocks[:, 1, None, None] + np.arange(8)[None, None, :]) + np.zeros((1, 8, 1), np.int64)
    report = []
    role_kw = dict(min_order=0, max_order=2, strict_nan=strict_nan, grid_role=L.GRID_TX if role == "tx" else L.GRID_RX, **kw)
    with Context(0) as c:
        c.set_scene(walls)
        got = c.value_and_grads(tx, X, Y, **role_kw)
        # The scene VJP sums over cells, and one cell anywhere in the grid with one of the reference's autodiff NaN artefacts
        # (un == 0 exactly: 22 cells of this grid, see test_cfg3_full_size_value_and_grad) makes the whole sum NaN -- in the
        # reference too, whatever the cotangent (0 * NaN).  The fixture's VJP is over its own cells only, so the GPU sweeps
        # exactly those: the blocks stacked into an (8 B) x 8 grid, one block per 8 x 8 patch of the kernel, which is culled
        # from the same bounding boxes as inside the full map.
        sub = c.value_and_grads(tx, X[ii, jj].reshape(-1, 8), Y[ii, jj].reshape(-1, 8), **role_kw)
    assert np.array_equal(got["value"][ii, jj], z["value"]), "value map differs from the oracle's on the fixture blocks"
    assert np.array_equal(sub["value"].reshape(z["value"].shape), z["value"])
    want = np.where(np.isnan(z["grad32"]), np.nan, z["grad"])  # fp64 values, fp32 NaN positions
    _tight(got["grad_rx"][ii, jj], want, z["grad32"], "per-cell gradient (inside the full grid)", report)
    _tight(sub["grad_rx"].reshape(want.shape), want, z["grad32"], "per-cell gradient (blocks alone)", report)
    _tight(sub["tx_bar"], np.where(np.isnan(z["fixed_bar32"]), np.nan, z["fixed_bar"]), z["fixed_bar32"], "VJP w.r.t. the fixed end point", report)
    _tight(sub["walls_bar"], np.where(np.isnan(z["walls_bar32"]), np.nan, z["walls_bar"]), z["walls_bar32"], "VJP w.r.t. the wall end points", report)
    assert np.abs(z["grad"]).max() > 1.0 and (z["value"] != 0).sum() >= 64  # the blocks do see paths
    print("\n".join(report))
