#!/usr/bin/env python3
"""Randomised differential test of the MinPath / FermatPath sweeps (GPU box): the solver kernels (K4) against
oracle/d2d_oracle_opt.c on random scenes of Wall / RIS / Vertex objects -- value maps and, every other case, per-cell gradients
through the solver loop -- orders 1..2 (order 3 in small scenes), both solvers, all validity modes, both grid roles, with
Adam (the reference's default) or SGD (plain, momentum, Nesterov, momentum 0.0: --optimizer sgd; mixed: either, per case).

Sequential fp32 Adam steps are not reproducible to the last bit between two gradient implementations and chaotic where a
solve has not settled, so cells are compared where the ORACLE ALONE calls the sweep well conditioned (CO.opt_conditioning:
every candidate's trajectory agrees between its fp64 run, its fp32 run and fp32 runs from inputs one ulp away); there the GPU
sits within 1e-5 of the map's scale (+ 1e-5 relative) of the fp64 oracle, or within four times the oracle's own fp32 distance.

usage: python scripts/fuzz_opt.py [--optimizer {adam,sgd,mixed}] [n_cases] [seed]"""

import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from differt2d_amd import _lib as L  # noqa: E402
from differt2d_amd.engine import Context  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402

F = np.float32
SGD_KINDS = ("plain", "momentum", "nesterov", "momentum0")


def random_sgd(rng, solver):
    """An optax.sgd for one case: (lr, momentum, nesterov).  Ranges where the oracle's own iteration is not chaotic: SGD does not
    normalise its step, and once lr times the objective's curvature exceeds 2 a solve jumps about and no two precisions follow
    it.  MinPath's residual has a curvature of order 1 / distance**2 next to a wall: lr in [5e-4, 2e-3] (tests/test_oracle_opt_c.py:
    at lr 0.005 .. 0.01 most order-2 solves of the RIS scene are chaotic after 50 steps); FermatPath's path length is tamer:
    lr in [2e-3, 1e-2].  Momentum in [0.1, 0.5]: a heavy trace at a large rate is chaotic too (tests/test_gpu_opt_sgd.py: 0.8 at
    lr 0.01)."""
    lo, hi = (5e-4, 2e-3) if solver == "min" else (2e-3, 1e-2)
    lr = float(F(np.exp(rng.uniform(np.log(lo), np.log(hi)))))
    kind = SGD_KINDS[int(rng.integers(0, len(SGD_KINDS)))]
    if kind == "plain":
        return kind, (lr, None, False)
    if kind == "momentum0":
        return kind, (lr, 0.0, False)
    return kind, (lr, float(F(rng.uniform(0.1, 0.5))), kind == "nesterov")


def random_case(rng):
    n = int(rng.integers(1, 7))
    kinds = rng.choice([0, 0, 0, 1, 2], n).astype(np.uint8)
    xys = rng.random((n, 2, 2)).astype(F)
    if rng.random() < 0.4:  # axis-aligned / lattice walls: receivers on supporting lines, collinear objects
        m = rng.random(xys.shape) < 0.5
        xys = np.where(m, np.round(xys * 4) / 4, xys).astype(F)
    xys[(xys[:, 0] == xys[:, 1]).all(-1)] += F(0.125)
    for j in range(n):
        if kinds[j] == 2:
            xys[j, 1] = xys[j, 0]
    phis = (rng.random(n) * 3.0 - 1.5).astype(F)
    fixed = rng.random(2).astype(F)
    gx, gy = int(rng.integers(1, 25)), int(rng.integers(1, 25))
    lo, hi = (-0.2, 1.2) if rng.random() < 0.3 else (0.0, 1.0)
    X, Y = np.meshgrid(np.linspace(lo, hi, gx).astype(F), np.linspace(lo, hi, gy).astype(F))
    mode = [(False, "hard_sigmoid"), (True, "hard_sigmoid"), (True, "sigmoid")][int(rng.integers(0, 3))]
    max_order = int(rng.integers(1, 4)) if n <= 3 else int(rng.integers(1, 3))
    min_order = int(rng.integers(0, max_order + 1))
    kw = dict(approx=mode[0], function=mode[1], alpha=float(rng.choice([100.0, 50.0, 10.0])), tol=float(rng.choice([1e-2, 1e-3, 0.5])),
              patch=float(rng.choice([0.0, 0.0, 0.02, -0.05])), fun=str(rng.choice(["received_power", "one", "length", "length_squared"])),
              solver=str(rng.choice(["min", "fermat"])), steps=int(rng.choice([1, 2, 5, 30, 100, 250])))
    cands = L.enumerate_candidates(n, min_order, max_order, None)
    theta0 = [rng.random(L.D2D_MAX_ORDER, dtype=F) for _ in cands]
    return kinds, xys, phis, fixed, X, Y, kw, min_order, max_order, cands, theta0


def check_case(ctx, case, kinds, xys, phis, fixed, X, Y, kw, min_order, max_order, cands, theta0, with_grad, role, sgd_spec=None):
    from differt2d_amd.optimize import sgd

    th = [t[: sum(kinds[int(i)] != 2 for i in c)] for c, t in zip(cands, theta0)]
    okw = {} if sgd_spec is None else CO.sgd_kwargs(*sgd_spec)
    cond = CO.opt_conditioning(kinds, xys, phis, fixed, X, Y, cands, th, kw["steps"], with_grad=with_grad,
                               grid_role="tx" if role == L.GRID_TX else "rx", **{k: v for k, v in kw.items() if k != "steps"}, **okw)
    ctx.set_optimizer(None if sgd_spec is None else sgd(sgd_spec[0], momentum=sgd_spec[1], nesterov=sgd_spec[2]))
    ctx.set_scene(xys, kinds, phis)
    ctx.set_theta0(theta0)
    gkw = dict(kw, min_order=min_order, max_order=max_order, grid_role=role)
    msgs = []
    if with_grad:
        out = ctx.value_and_grads(fixed, X, Y, **gkw)
        got, g = out["value"], out["grad_rx"].astype(np.float64)
        if not np.array_equal(got, ctx.power_map(fixed, X, Y, **gkw), equal_nan=True):
            msgs.append("value map of the gradient sweep differs from the forward sweep's")
    else:
        got = ctx.power_map(fixed, X, Y, **gkw)
    stable, v64, scale = cond["stable"], cond["value64"], cond["scale"]
    # (four times the oracle's own fp32-to-fp64 distance: a cell that amplifies rounding a hundredfold does so for every fp32
    # evaluation, and by a factor that varies from one evaluation order to the next)
    bar = np.maximum(1e-5 * scale + 1e-5 * np.abs(v64), 4.0 * cond["dist"]) + 1e-30
    ok = np.abs(got - v64) <= bar
    # a solver left in Adam's period-2 limit cycle: either of its two points (CO.opt_conditioning, `parity`)
    ok |= cond["parity"] & (np.abs(got - cond["value32_next"]) <= bar + cond["dist"])
    bad = stable & ~ok
    if bad.any():
        w = tuple(np.argwhere(bad)[0])
        msgs.append(f"value ({int(bad.sum())} of {int(stable.sum())} stable cells, first {w}: GPU {got[w]!r} oracle64 {v64[w]!r} oracle32 {cond['value32'][w]!r})")
    n_grad = 0
    if with_grad:
        g64, g32, g32t, g32n = cond["grad64"], cond["grad32"], cond["grad32t"], cond["grad32n"]
        fin = np.isfinite(g64).all(-1) & np.isfinite(g32).all(-1) & np.isfinite(g32n).all(-1) & stable & ~cond["parity"]
        with np.errstate(invalid="ignore"):
            # a cell's gradient scale: its own largest component, at least 1e-2 of the map's (contributions of opposite sign cancel)
            gs = np.maximum(np.abs(np.nan_to_num(g64)).max(-1), 1e-2 * float(np.nanmax(np.abs(np.where(np.isfinite(g64), g64, 0.0)), initial=0.0)) + 1e-30)[..., None]
            # the gradient through the loop must itself be well conditioned: the oracle's fp32 run, and its fp32 run from a cell one
            # ulp away, within 1e-2 of the cell's scale of its fp64 run
            fin &= (np.abs(g32 - g64) <= 1e-2 * gs).all(-1) & (np.abs(g32n - g64) <= 1e-2 * gs).all(-1)
            # 3e-5 of the cell's gradient scale (fp32 reverse mode through up to 250 sequential Adam steps: the reference chain's own
            # fp32 reverse mode sits 1 .. 4e-5 from its fp64 one in these cases, scripts/fuzz_opt_case.py), or twice what the oracle's
            # own fp32 runs lose (values in fp32; derivatives in fp32 too; one input ulp)
            gbar = np.maximum(3e-5 * gs + 1e-5 * np.abs(g64), 2.0 * np.maximum(np.maximum(np.abs(g32 - g64), np.nan_to_num(np.abs(g32t - g64))), np.abs(g32n - g64)))
            gbad = fin & ~(np.abs(g - g64) <= gbar).all(-1)
        n_grad = int(fin.sum())
        # offenders: the yardstick of tests/test_gpu_opt.py -- the reference chain's OWN fp32 reverse mode through the loop
        # (oracle/ref.py under torch) on that cell: within twice ITS distance from fp64
        if gbad.any() and gbad.sum() <= 32:
            from oracle import ref as R
            from contextlib import nullcontext

            rkw = dict(solver=kw["solver"], steps=kw["steps"], approx=kw["approx"], alpha=kw["alpha"], tol=kw["tol"], patch=kw["patch"], fun=kw["fun"],
                       grid_role="tx" if role == L.GRID_TX else "rx", **({"function": kw["function"]} if kw["approx"] else {}))
            wb = np.argwhere(gbad)
            print(f"  .. case {case}: {len(wb)} cells to the reverse-mode yardstick", flush=True)
            Xc, Yc = X[wb[:, 0], wb[:, 1]][None], Y[wb[:, 0], wb[:, 1]][None]  # (one batched call per precision)
            with R.sgd_hyper(*sgd_spec) if sgd_spec is not None else nullcontext():
                t = {dt: R.opt_value_and_grads(kinds, np.asarray(xys, np.float64), phis, fixed, Xc, Yc, cands, th, dtype=dt, **rkw)["grad_cell"][0]
                     for dt in ("float64", "float32")}
            for i, w in enumerate(map(tuple, wb)):
                # (as vectors, and five times the reference chain's own fp32-reverse-mode distance: two different backward passes in
                # fp32 -- torch's and the kernels' -- sit at different multiples of the same rounding; seed 2 case 193, sigmoid in deep
                # shadow: torch 2.2e-5 of the cell's scale off fp64, the kernels 9.5e-5)
                if np.isfinite(t["float32"][i]).all() and np.linalg.norm(g[w] - t["float64"][i]) <= np.linalg.norm(gbar[w]) + 5.0 * np.linalg.norm(t["float32"][i] - t["float64"][i]):
                    gbad[w] = False
        if gbad.any():
            w = tuple(np.argwhere(gbad)[0])
            msgs.append(f"gradient ({int(gbad.sum())} of {n_grad} cells, first {w}: GPU {g[w]} oracle64 {g64[w]} oracle32 {g32[w]})")
    return msgs, int(stable.sum()), int(stable.size), n_grad


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--optimizer", choices=("adam", "sgd", "mixed"), default="adam")
    ap.add_argument("n_cases", nargs="?", type=int, default=200)
    ap.add_argument("seed", nargs="?", type=int, default=0)
    args = ap.parse_args()
    n_cases, seed = args.n_cases, args.seed
    rng = np.random.default_rng(seed)
    bad = n_stable = n_cells = n_grad = 0
    t0 = time.time()
    with Context(0) as ctx:
        for case in range(n_cases):
            kinds, xys, phis, fixed, X, Y, kw, lo, hi, cands, theta0 = random_case(rng)
            role = L.GRID_TX if case % 3 == 2 else L.GRID_RX
            opt, sgd_spec = "adam", None
            # (drawn from a generator of their own: the Adam cases of a seed stay the cases they always were)
            if args.optimizer == "sgd" or (args.optimizer == "mixed" and case % 2 == 0):
                opt, sgd_spec = random_sgd(np.random.default_rng([seed, case]), kw["solver"])
            msgs, s, c, g = check_case(ctx, case, kinds, xys, phis, fixed, X, Y, kw, lo, hi, cands, theta0, case % 2 == 1, role, sgd_spec)
            n_stable, n_cells, n_grad = n_stable + s, n_cells + c, n_grad + g
            if msgs:
                bad += 1
                print(f"MISMATCH case {case} seed {seed} {'TX' if role == L.GRID_TX else 'RX'}-grid: kinds={kinds.tolist()} grid={X.shape} orders {lo}..{hi} "
                      f"kw={kw} optimizer {opt} {sgd_spec}: " + "; ".join(msgs), flush=True)
            if case % 100 == 99:
                print(f"  .. {case + 1} cases, {bad} mismatches, {n_stable} of {n_cells} cells well conditioned, {n_grad} gradients compared, {time.time() - t0:.0f} s", flush=True)
    print(f"opt fuzz ({args.optimizer}): {n_cases} cases, {bad} mismatches, {n_stable} of {n_cells} cells well conditioned (values compared there), "
          f"{n_grad} per-cell gradients compared, {time.time() - t0:.1f} s (seed {seed})")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
