"""What does the per-cell channel matrix cost?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024 cells, orders 0..2),
wavelength 0.05, half-wavelength uniform linear arrays of 1 x 1, 2 x 2, 4 x 4 and 8 x 8 elements, hard and hard_sigmoid validity, both
grid roles.  Per leg, on ONE context in ONE process: the four array-response launches (d2d_array_response_launch: the zeroing of the
2 nr nt planes and power_sink_kernel with an ArraySink) beside one coherent-field launch (the yardstick of the 1 x 1 matrix: a FieldSink
in the same kernel, no zeroing) and the frequency-response launches with nf = nr nt wavelengths (what a design that keeps 8 planes in
registers per pass would cost: ceil(nr nt / 8) whole sweeps), interleaved in blocks so that clock drift hits all alike -- HIP events
around a block of back-to-back launches, median over the blocks of the per-launch time, and the blocks' own spread.  Before anything is
timed the 1 x 1 matrix (a zero offset at both ends) is held to the coherent field and every total to the fused map, bit for bit.
Every leg is a child process of its own under its own time limit; the first leg that fails ends the run.

    python scripts/array_response_bench.py [--out profiles/array_response_bench.txt] [--blocks 4] [--steps 30] [--warmup 5]
"""

import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WAVELENGTH = 0.05
SIZES = [1, 2, 4, 8]  # n x n
LEGS = [("rx", "hard"), ("rx", "hard_sigmoid"), ("tx", "hard"), ("tx", "hard_sigmoid")]
LEG_SECONDS = 240


def leg(role, mode, blocks, steps, warmup):
    from conftest import random_scene
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context, make_params
    from differt2d_amd.utils import ula

    F = np.float32
    fixed, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    inv = F(1) / F(WAVELENGTH)
    params = make_params(min_order=0, max_order=2, approx=mode != "hard", function="hard_sigmoid",
                         grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    arrays = {n: (ula(n, WAVELENGTH / 2), ula(n, WAVELENGTH / 2, np.pi / 2)) for n in SIZES}
    with Context(0) as c:
        c.set_scene(walls)
        c.set_grid(X, Y)
        run = {"fused": lambda: c.launch(params, fixed), "field": lambda: c.launch_coherent_field(params, fixed, inv, "sqrt")}
        for n in SIZES:
            run[f"array{n}"] = lambda n=n: c.launch_array_response(params, fixed, inv, arrays[n][0], arrays[n][1], "sqrt")
            run[f"freq{n * n}"] = lambda n=n: c.launch_frequency_response(params, fixed, np.full(n * n, inv, F), "sqrt")
        for f in run.values():  # warm-up: code objects, masks, lists, work history, the outputs' buffers
            for _ in range(warmup):
                f()
        c.synchronize()
        # what is timed computes what it should: the 1 x 1 matrix (ula(1) is a zero offset) is the coherent field by bits -- but for a
        # cell that is the fixed end point itself, whose line of sight has no direction -- and every total is the fused map
        c.launch(params, fixed)
        fused = c.get_map()
        cf = c.coherent_field(params, fixed, inv, "sqrt")
        one = c.array_response(params, fixed, inv, *arrays[1], "sqrt")
        assert np.array_equal(bits(one.total), bits(fused)) and np.array_equal(bits(cf.total), bits(fused))
        assert np.array_equal(bits(one.im[0, 0]), bits(cf.im)) and (bits(one.re[0, 0]) != bits(cf.re)).sum() <= 1
        four = c.array_response(params, fixed, inv, *arrays[4], "sqrt")
        assert four.re.shape == (4, 4, 1024, 1024) and np.array_equal(bits(four.total), bits(fused))
        lit = float((fused != 0).mean())
        distinct = all(not np.array_equal(bits(four.im[i, j]), bits(four.im[0, 0])) for i in range(4) for j in range(4) if (i, j) != (0, 0))
        assert distinct
        del four
        ms = {k: [] for k in run}
        for _ in range(blocks):
            for k, f in run.items():
                c.timer_begin()
                for _ in range(steps):
                    f()
                ms[k].append(c.timer_end() / steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    span = lambda k: f"{min(ms[k]):.4f} .. {max(ms[k]):.4f}"
    out = [f"{role} {mode:13s} fused sweep {med['fused']:.4f} ms   coherent field {med['field']:.4f} ms (blocks {span('field')})"]
    for n in SIZES:
        a, f = med[f"array{n}"], med[f"freq{n * n}"]
        out.append(f"    {n} x {n}: array response {a:.4f} ms (blocks {span(f'array{n}')}; x{a / med['field']:.2f} the coherent field)   "
                   f"frequency response nf = {n * n} {f:.4f} ms (blocks {span(f'freq{n * n}')})   array / frequency x{a / f:.2f}")
    out.append(f"    [{blocks} x {steps} launches each; {100 * lit:.1f} % of the cells lit; the 1 x 1 matrix equals the coherent field and every "
               f"total the fused map by bits; the 16 planes of 4 x 4 differ]")
    print("\n".join(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "array_response_bench.txt"))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--leg", nargs=2, metavar=("ROLE", "MODE"), help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg[0], args.leg[1], args.blocks, args.steps, args.warmup)
        return
    lines = [f"array response beside the coherent field and the frequency response with nf = nr nt: configs[1] (50 walls, 1024 x 1024, orders "
             f"0..2), received_power, wavelength {WAVELENGTH:g}, half-wavelength ULAs (transmit along x, receive along y), amplitude sqrt, one "
             f"context per leg, {args.blocks} interleaved blocks of {args.steps} launches ({args.blocks * args.steps} timed steps), median ms "
             f"per launch and the blocks' range"]
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
