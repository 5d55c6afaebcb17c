"""What does the per-cell power-angle profile cost?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024 cells, orders 0..2),
36 bins from origin 0, at the receiver and at the transmitter, hard and hard_sigmoid validity, both grid roles.  Per leg, on ONE
context in ONE process: the two power-angle launches (d2d_power_angle_launch: the zeroing of the planes and power_sink_kernel with
an AngleSink) beside the 32-bin power-delay profile launch of the same parameters (the yardstick: a BinSink in the same kernel) and
the fused sweep, interleaved in blocks so that clock drift hits all alike -- HIP events around a block of back-to-back launches,
median over the blocks of the per-launch time, and the blocks' own spread -- and beside ONE record pass of d2d_valid_paths (pass 1,
the library's own events).  Before anything is timed the total plane and a one-bin launch are held to the fused map, bit for bit.
Every leg is a child process of its own under its own time limit; the first leg that fails ends the run.

    python scripts/power_angle_bench.py [--out profiles/power_angle_bench.txt] [--blocks 4] [--steps 50] [--warmup 10]
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

NBINS = 36
PROFILE_NBINS, R_MIN, R_MAX = 32, 0.0, 4.0
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
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    with Context(0) as c:
        c.set_scene(walls)
        c.set_grid(X, Y)
        c.set_option("time_kernel", 1)
        run = {"fused": lambda: c.launch(params, fixed),
               "profile": lambda: c.launch_profile(params, fixed, R_MIN, R_MAX, PROFILE_NBINS),
               "angle_rx": lambda: c.launch_power_angle(params, fixed, "rx", 0.0, NBINS),
               "angle_tx": lambda: c.launch_power_angle(params, fixed, "tx", 0.0, NBINS)}
        for f in run.values():  # warm-up: code objects, masks, lists, work history, the outputs' buffers
            for _ in range(warmup):
                f()
        c.synchronize()
        # what is timed computes what it should: total and a one-bin launch are the fused map by bits, and the 36 bins of a cell
        # sum to it up to fp32 summation order
        c.launch(params, fixed)
        fused = c.get_map()
        used = {}
        for at in ("rx", "tx"):
            one = c.power_angle(params, fixed, at, 0.0, 1)
            assert np.array_equal(bits(one.total), bits(fused)) and np.array_equal(bits(one.bins[0]), bits(fused)), at
            pa = c.power_angle(params, fixed, at, 0.0, NBINS)
            assert np.array_equal(bits(pa.total), bits(fused)), at
            s = pa.bins.astype(np.float64).sum(0)
            assert np.allclose(s, fused, rtol=1e-5, atol=1e-6 * float(fused.max())), (at, float(np.abs(s - fused).max()))
            lit = fused != 0
            used[at] = float(((pa.bins != 0).sum(0) >= 2)[lit].mean())
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
    med = {k: float(np.median(v)) for k, v in ms.items()}
    r = float(np.median(rec))
    p = med["profile"]
    span = lambda k: f"{min(ms[k]):.4f} .. {max(ms[k]):.4f}"
    print(f"{role} {mode:13s} fused sweep {med['fused']:.4f} ms   record pass 1 {r:.4f} ms   delay profile ({PROFILE_NBINS} bins) {p:.4f} ms "
          f"(blocks {span('profile')})   power-angle profile ({NBINS} bins): at rx {med['angle_rx']:.4f} ms (blocks {span('angle_rx')}; "
          f"x{med['angle_rx'] / p:.2f} the delay profile, x{med['angle_rx'] / r:.2f} one record pass)   at tx {med['angle_tx']:.4f} ms "
          f"(blocks {span('angle_tx')}; x{med['angle_tx'] / p:.2f} the delay profile, x{med['angle_tx'] / r:.2f} one record pass)   "
          f"[{blocks} x {steps} launches each; {n.value} records; lit cells with power in two or more bins: {100 * used['rx']:.1f} % at rx, "
          f"{100 * used['tx']:.1f} % at tx; total and one bin equal the fused map by bits]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_angle_bench.txt"))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--leg", nargs=2, metavar=("ROLE", "MODE"), help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg[0], args.leg[1], args.blocks, args.steps, args.warmup)
        return
    lines = [f"power-angle profile beside the power-delay profile, the fused sweep and one record pass: configs[1] (50 walls, 1024 x 1024, "
             f"orders 0..2), received_power, {NBINS} angle bins from origin 0, {PROFILE_NBINS} delay bins over [{R_MIN:g}, {R_MAX:g}), one "
             f"context per leg, {args.blocks} interleaved blocks of {args.steps} launches ({args.blocks * args.steps} timed steps), median "
             f"ms per launch and the blocks' range"]
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
