"""What does the per-cell power-delay profile cost?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024 cells, orders 0..2),
32 bins over [0, 4), hard and hard_sigmoid validity, both grid roles.  Per leg, on ONE context in ONE process: the profile launch
(d2d_power_profile_launch: the zeroing of the profile and power_sink_kernel with a BinSink) beside the fused sweep of the same parameters,
interleaved in blocks so that clock drift hits both alike -- HIP events around a block of back-to-back launches, median over the
blocks of the per-launch time -- and beside ONE record pass of d2d_valid_paths (pass 1, the library's own events: the same
enumeration in the same launch shape with a record sink).  Every leg is a child process of its own under its own time limit; the
first leg that fails ends the run.

    python scripts/power_profile_bench.py [--out profiles/power_profile_bench.txt] [--blocks 4] [--steps 50] [--warmup 10]
"""

import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NBINS, R_MIN, R_MAX = 32, 0.0, 4.0
LEGS = [("rx", "hard"), ("rx", "hard_sigmoid"), ("tx", "hard"), ("tx", "hard_sigmoid")]
LEG_SECONDS = 240


def leg(role, mode, blocks, steps, warmup):
    from conftest import random_scene
    from differt2d_amd import _lib as L
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
        run = {"fused": lambda: c.launch(params, fixed), "profile": lambda: c.launch_profile(params, fixed, R_MIN, R_MAX, NBINS)}
        for f in run.values():  # warm-up: code objects, masks, lists, work history, the profile's buffer
            for _ in range(warmup):
                f()
        c.synchronize()
        # what is timed computes what it should: over a range that covers every path the bins of a cell sum to the fused value
        c.launch(params, fixed)
        fused = c.get_map().astype(np.float64)
        cover = c.power_profile(params, fixed, 0.0, 16.0, NBINS).astype(np.float64).sum(0)
        dev = float(np.abs(cover - fused).max())
        assert np.allclose(cover, fused, rtol=1e-5, atol=1e-6 * fused.max()), dev
        inside = float(c.power_profile(params, fixed, R_MIN, R_MAX, NBINS).astype(np.float64).sum() / fused.sum())
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
    a, b, r = float(np.median(ms["fused"])), float(np.median(ms["profile"])), float(np.median(rec))
    print(f"{role} {mode:13s} fused sweep {a:.4f} ms   profile launch {b:.4f} ms (min {min(ms['profile']):.4f}; x{b / a:.2f} the fused sweep, "
          f"x{b / r:.2f} one record pass)   record pass 1 {r:.4f} ms   [{blocks} x {steps} launches each; {n.value} records; "
          f"{100 * inside:.2f} % of the power inside [{R_MIN:g}, {R_MAX:g}); max |sum of bins - fused| {dev:.3g}]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_profile_bench.txt"))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--leg", nargs=2, metavar=("ROLE", "MODE"), help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg[0], args.leg[1], args.blocks, args.steps, args.warmup)
        return
    lines = [f"power-delay profile beside the fused sweep and one record pass: configs[1] (50 walls, 1024 x 1024, orders 0..2), {NBINS} bins "
             f"over [{R_MIN:g}, {R_MAX:g}), one context per leg, {args.blocks} interleaved blocks of {args.steps} launches "
             f"({args.blocks * args.steps} timed steps), median ms per launch"]
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
