"""What does the coherent field cost?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024 cells, orders 0..2),
received_power, wavelength 0.05, both amplitude modes.  Per leg (grid role x validity), on ONE context in ONE process: the
coherent-field launch (d2d_coherent_field_launch: power_sink_kernel with a FieldSink) beside the fused sweep of the same parameters
and the strongest-paths launch at k = 1 and k = 8 (the same kernel with a TopSink), interleaved in blocks so that clock drift hits
all alike -- HIP events around a block of back-to-back launches, median over the blocks of the per-launch time -- and beside ONE
record pass of d2d_valid_paths (pass 1, the library's own events: the same enumeration in the same launch shape with a record
sink).  Every leg is a child process of its own under its own time limit; the first leg that fails ends the run.

    python scripts/coherent_field_bench.py [--out profiles/coherent_field_bench.txt] [--blocks 4] [--steps 50] [--warmup 10]
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

LEGS = [("rx", "hard"), ("rx", "hard_sigmoid"), ("tx", "hard"), ("tx", "hard_sigmoid")]
LEG_SECONDS = 240
WAVELENGTH = 0.05


def leg(role, mode, blocks, steps, warmup):
    from conftest import random_scene
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context, make_params
    from differt2d_amd.utils import fading_gain

    F = np.float32
    fixed, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    inv = F(1) / F(WAVELENGTH)
    params = make_params(min_order=0, max_order=2, approx=mode != "hard", function="hard_sigmoid",
                         grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)
    with Context(0) as c:
        c.set_scene(walls)
        c.set_grid(X, Y)
        c.set_option("time_kernel", 1)
        run = {
            "fused": lambda: c.launch(params, fixed),
            "top1": lambda: c.launch_strongest_paths(params, fixed, 1),
            "top8": lambda: c.launch_strongest_paths(params, fixed, 8),
            "sqrt": lambda: c.launch_coherent_field(params, fixed, inv, "sqrt"),
            "linear": lambda: c.launch_coherent_field(params, fixed, inv, "linear"),
        }
        for f in run.values():  # warm-up: code objects, masks, lists, work history, the results' buffers
            for _ in range(warmup):
                f()
        c.synchronize()
        # what is timed computes what it should: total is the fused map bit for bit, and so is re at an infinite wavelength
        c.launch(params, fixed)
        fused = c.get_map()
        cf = c.coherent_field(params, fixed, inv, "sqrt")
        assert np.array_equal(cf.total.view(np.uint32), fused.view(np.uint32))
        flat = c.coherent_field(params, fixed, 0.0, "linear")
        assert np.array_equal(flat.re.view(np.uint32), fused.view(np.uint32)) and not flat.im.view(np.uint32).any()
        gain = fading_gain(cf)
        lit = np.isfinite(gain)
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
    fields = "   ".join(f"{k} {med[k]:.4f} ms (x{med[k] / med['fused']:.2f} fused, x{med[k] / r:.2f} record pass, x{med[k] / med['top8']:.2f} top-8)"
                        for k in ("sqrt", "linear"))
    print(f"{role} {mode:13s} fused sweep {med['fused']:.4f} ms   record pass 1 {r:.4f} ms   strongest paths k=1 {med['top1']:.4f} ms  k=8 "
          f"{med['top8']:.4f} ms   coherent field: {fields}   [{blocks} x {steps} launches each; {int(n.value)} records; fading gain "
          f"|field|^2 / total over the {int(lit.sum())} lit cells: median {float(np.median(gain[lit])):.3f}, "
          f"{100 * float((gain[lit] < 0.5).mean()):.1f} % below 0.5, {100 * float((gain[lit] > 1.5).mean()):.1f} % above 1.5]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coherent_field_bench.txt"))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--leg", nargs=2, metavar=("ROLE", "MODE"), help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg[0], args.leg[1], args.blocks, args.steps, args.warmup)
        return
    lines = [f"coherent field beside the fused sweep, one record pass and the strongest paths: configs[1] (50 walls, 1024 x 1024, orders "
             f"0..2), received_power, wavelength {WAVELENGTH}, one context per leg, {args.blocks} interleaved blocks of {args.steps} "
             f"launches ({args.blocks * args.steps} timed steps), median ms per launch"]
    for role, mode in LEGS:  # (this process never opens the GPU: each leg is a fresh child under its own time limit)
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", role, mode, "--blocks", str(args.blocks), "--steps", str(args.steps),
               "--warmup", str(args.warmup)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LEG_SECONDS)
        print(done.stdout, end="", flush=True)
        lines += done.stdout.splitlines()
        if done.returncode != 0:
            failed = f"leg {role} {mode} ended with status {done.returncode}: stopping"
            lines.append(failed)
            break
    else:
        failed = None
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    if failed:
        sys.exit(failed)


if __name__ == "__main__":
    main()
