"""What do the per-cell strongest paths cost?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024 cells, orders 0..2),
k = 1, 4 and 8, received_power.  Per leg, on ONE context in ONE process: the top-k launch (d2d_strongest_paths_launch:
power_sink_kernel with a TopSink) beside the fused sweep of the same parameters, interleaved in blocks so that clock drift hits all
alike -- HIP events around a block of back-to-back launches, median over the blocks of the per-launch time -- beside ONE record
pass of d2d_valid_paths (pass 1, the library's own events: the same enumeration in the same launch shape with a record sink), and
beside the whole of the route that exists without the feature, wall clock: Context.valid_paths, then on the host the path function
from the records' lengths and orders, a sort by (cell, magnitude descending) and the cut to k.  Every leg is a child process of its
own under its own time limit; the first leg that fails ends the run.

    python scripts/strongest_paths_bench.py [--out profiles/strongest_paths_bench.txt] [--blocks 4] [--steps 50] [--warmup 10]
"""

import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KS = (1, 4, 8)
LEGS = [("rx", "hard"), ("rx", "hard_sigmoid"), ("tx", "hard")]
LEG_SECONDS = 240


def records_route(c, params, fixed, cells, k, r_coef, height):
    """The k strongest paths per cell from the sparse records: (power [k, cells], seconds of the call, seconds on the host)."""
    F = np.float32
    t0 = time.perf_counter()
    rec = c.valid_paths(params, fixed)
    t1 = time.perf_counter()
    r = rec["length"]
    t = (rec["valid"] * (F(r_coef) ** rec["order"]).astype(F) / (F(height) * F(height) + r * r)).astype(F)
    key = np.abs(t).view(np.uint32).astype(np.int64)
    by = np.lexsort((-key, rec["cell"]))  # (stable: equal keys stay in record order)
    cell = rec["cell"][by]
    slot = np.arange(by.size) - np.searchsorted(cell, cell, side="left")
    keep = slot < k
    power = np.zeros((k, cells), F)
    power[slot[keep], cell[keep]] = t[by][keep]
    t2 = time.perf_counter()
    return power, t1 - t0, t2 - t1, len(r)


def leg(role, mode, blocks, steps, warmup):
    from conftest import random_scene
    from differt2d_amd import _lib as L
    from differt2d_amd.defaults import DEFAULT_HEIGHT, DEFAULT_R_COEF
    from differt2d_amd.engine import Context, make_params

    F = np.float32
    fixed, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    params = make_params(min_order=0, max_order=2, approx=mode != "hard", function="hard_sigmoid",
                         grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)
    with Context(0) as c:
        c.set_scene(walls)
        c.set_grid(X, Y)
        c.set_option("time_kernel", 1)
        run = {"fused": lambda: c.launch(params, fixed)}
        for k in KS:
            run[f"top{k}"] = lambda k=k: c.launch_strongest_paths(params, fixed, k)
        for f in run.values():  # warm-up: code objects, masks, lists, work history, the result's buffers
            for _ in range(warmup):
                f()
        c.synchronize()
        # what is timed computes what it should: total is the fused map bit for bit, and the slots are the records route's
        c.launch(params, fixed)
        fused = c.get_map()
        sp = c.strongest_paths(params, fixed, 8)
        assert np.array_equal(sp.total.view(np.uint32), fused.view(np.uint32))
        route = []
        for _ in range(1 + 3):
            power, call_s, host_s, n_rec = records_route(c, params, fixed, X.size, 8, DEFAULT_R_COEF, DEFAULT_HEIGHT)
            route.append((call_s, host_s))
        route = route[1:]
        dev = float(np.abs(power.reshape(sp.power.shape).astype(np.float64) - sp.power).max())
        assert np.allclose(power.reshape(sp.power.shape), sp.power, rtol=1e-5, atol=1e-6 * float(sp.power.max())), dev
        cut = float((sp.count > 8).mean())
        ms = {k: [] for k in run}
        for _ in range(blocks):
            for k, f in run.items():
                c.timer_begin()
                for _ in range(steps):
                    f()
                ms[k].append(c.timer_end() / steps)
        rec = []
        n = ctypes.c_int64(0)
        for _ in range(5 + 15):
            L.check(c._lib.d2d_valid_paths(c._ctx, ctypes.byref(params), np.ascontiguousarray(fixed, F), ctypes.byref(n)))
            rec.append(c.valid_paths_ms()["count_ms"])
        rec = rec[5:]
    a, r = float(np.median(ms["fused"])), float(np.median(rec))
    call_ms = 1e3 * float(np.median([x[0] for x in route]))
    host_ms = 1e3 * float(np.median([x[1] for x in route]))
    tops = "   ".join(f"k={k} {float(np.median(ms[f'top{k}'])):.4f} ms (x{float(np.median(ms[f'top{k}'])) / a:.2f} fused, "
                      f"x{float(np.median(ms[f'top{k}'])) / r:.2f} record pass)" for k in KS)
    print(f"{role} {mode:13s} fused sweep {a:.4f} ms   record pass 1 {r:.4f} ms   top-k launch: {tops}   records route (k = 8): "
          f"valid_paths {call_ms:.2f} ms + host sort and cut {host_ms:.2f} ms   [{blocks} x {steps} launches each; {n_rec} records; "
          f"{100 * cut:.2f} % of the cells have more than 8 paths; max |route - slots| {dev:.3g}]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strongest_paths_bench.txt"))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--leg", nargs=2, metavar=("ROLE", "MODE"), help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg[0], args.leg[1], args.blocks, args.steps, args.warmup)
        return
    lines = [f"per-cell strongest paths beside the fused sweep, one record pass and the records route: configs[1] (50 walls, 1024 x 1024, "
             f"orders 0..2), k = {', '.join(map(str, KS))}, one context per leg, {args.blocks} interleaved blocks of {args.steps} launches "
             f"({args.blocks * args.steps} timed steps), median ms per launch; the records route is wall clock, median of 3 calls"]
    for role, mode in LEGS:  # (this process never opens the GPU: each leg is a fresh child under its own time limit)
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", role, mode, "--blocks", str(args.blocks), "--steps", str(args.steps),
               "--warmup", str(args.warmup)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LEG_SECONDS)
        print(done.stdout, end="", flush=True)
        if done.returncode != 0:
            sys.exit(f"leg {role} {mode} ended with status {done.returncode}: stopping")
        lines += done.stdout.splitlines()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
