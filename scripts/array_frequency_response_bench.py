"""What does the wideband channel tensor cost beside the calls it replaces?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024
cells, orders 0..2), half-wavelength uniform linear arrays of 1 x 1, 2 x 2, 4 x 4 and 8 x 8 elements at nf = 1, 8 and 64 inverse
wavelengths 20 + k / 32, hard and hard_sigmoid validity, both grid roles.  Per leg, on ONE context in ONE process: the wideband launch
(d2d_array_frequency_response_launch: one preparation, the zeroing of the 2 nf nr nt planes and ceil(nf / WIDE_CHUNK) passes of
power_sink_kernel with an ArrayFreqSink) beside the route it replaces -- nf d2d_array_response_launch calls, one per entry of the same
list, each with its own check, preparation, zeroing and sweep -- and beside one such call, interleaved in blocks so that clock drift
hits all alike: HIP events around a block of back-to-back calls, median over the blocks of the per-call time, and the blocks' own
spread.  Shapes of more than 64 planes run fewer calls per block (the line says how many).  Before anything is timed, after a warm-up
of every shape, the first and the last plane block of every wideband result are held to Context.array_response's bits.  Every leg is
a child process of its own under its own time limit; the first leg that fails ends the run.

    python scripts/array_frequency_response_bench.py [--out profiles/array_frequency_response_bench.txt] [--blocks 4] [--steps 20] [--warmup 2]
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
COUNTS = [1, 8, 64]   # nf
LEGS = [("rx", "hard"), ("rx", "hard_sigmoid"), ("tx", "hard"), ("tx", "hard_sigmoid")]
LEG_SECONDS = 420


def calls_per_block(steps, n, nf):
    """`steps` up to 64 planes, fewer in proportion above, never under 3."""
    return max(3, min(steps, steps * 64 // (n * n * nf)))


def leg(role, mode, blocks, steps, warmup, sizes, counts):
    from conftest import random_scene
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context, make_params
    from differt2d_amd.utils import ula

    F = np.float32
    fixed, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    inv = {nf: (F(20) + np.arange(nf, dtype=F) / F(32)).astype(F) for nf in counts}
    params = make_params(min_order=0, max_order=2, approx=mode != "hard", function="hard_sigmoid",
                         grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    arrays = {n: (ula(n, WAVELENGTH / 2), ula(n, WAVELENGTH / 2, np.pi / 2)) for n in sizes}
    with Context(0) as c:
        c.set_scene(walls)
        c.set_grid(X, Y)

        def repeat(n, nf):
            for v in inv[nf]:
                c.launch_array_response(params, fixed, v, arrays[n][0], arrays[n][1], "sqrt")

        run = {}
        for n in sizes:
            run[("one", n, 1)] = lambda n=n: c.launch_array_response(params, fixed, inv[counts[0]][0], arrays[n][0], arrays[n][1], "sqrt")
            for nf in counts:
                run[("wide", n, nf)] = lambda n=n, nf=nf: c.launch_array_frequency_response(params, fixed, inv[nf], arrays[n][0], arrays[n][1], "sqrt")
                if nf > 1:
                    run[("repeat", n, nf)] = lambda n=n, nf=nf: repeat(n, nf)
        for f in run.values():  # warm-up of every shape: code objects, masks, lists, work history, the outputs' buffers
            for _ in range(warmup):
                f()
        c.synchronize()
        # what is timed computes what it should: the first and the last plane block of every result are the array response's bits
        c.launch(params, fixed)
        fused = c.get_map()
        lit = float((fused != 0).mean())
        for n in sizes:
            for nf in counts:
                run[("wide", n, nf)]()
                for f in sorted({0, nf - 1}):
                    got = c.get_array_frequency_response(f, 1)
                    want = c.array_response(params, fixed, inv[nf][f], arrays[n][0], arrays[n][1], "sqrt")
                    assert got.re.shape == (1, n, n, 1024, 1024) and want.im.any()
                    assert np.array_equal(bits(got.re[0]), bits(want.re)) and np.array_equal(bits(got.im[0]), bits(want.im)), (n, nf, f)
                    assert np.array_equal(bits(got.total), bits(want.total)) and np.array_equal(bits(got.total), bits(fused)), (n, nf, f)
                    del got, want
        ms = {k: [] for k in run}
        for _ in range(blocks):
            for k, f in run.items():
                reps = calls_per_block(steps, k[1], k[2])
                c.timer_begin()
                for _ in range(reps):
                    f()
                ms[k].append(c.timer_end() / reps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    span = lambda k: f"{min(ms[k]):.3f} .. {max(ms[k]):.3f}"
    out = [f"{role} {mode:13s} ({100 * lit:.1f} % of the cells lit; first and last plane block of every result equal Context.array_response by bits)"]
    for n in sizes:
        one = med[("one", n, 1)]
        out.append(f"    {n} x {n}: one array_response launch {one:.3f} ms (blocks {span(('one', n, 1))})")
        for nf in counts:
            w = med[("wide", n, nf)]
            r, rspan = (med[("repeat", n, nf)], span(("repeat", n, nf))) if nf > 1 else (one, span(("one", n, 1)))
            faster = max(ms[("wide", n, nf)]) < (min(ms[("repeat", n, nf)]) if nf > 1 else min(ms[("one", n, 1)]))
            out.append(f"        nf = {nf:2d}: wideband {w:9.3f} ms (blocks {span(('wide', n, nf))})   {nf:2d} array_response launches {r:9.3f} ms "
                       f"(blocks {rspan})   x{w / r:.3f}   {'every block faster' if faster else 'NOT faster in every block'}   "
                       f"[{calls_per_block(steps, n, nf)} calls per block]")
    print("\n".join(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "array_frequency_response_bench.txt"))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
    ap.add_argument("--counts", type=int, nargs="+", default=COUNTS)
    ap.add_argument("--legs", type=int, nargs="+", default=list(range(len(LEGS))), help="indices into the four legs")
    ap.add_argument("--leg", nargs=2, metavar=("ROLE", "MODE"), help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg[0], args.leg[1], args.blocks, args.steps, args.warmup, args.sizes, args.counts)
        return
    lines = [f"wideband array response beside the array_response launches it replaces: configs[1] (50 walls, 1024 x 1024, orders 0..2), "
             f"received_power, inverse wavelengths 20 + k / 32, half-wavelength ULAs (transmit along x, receive along y), amplitude sqrt, one "
             f"context per leg, {args.blocks} interleaved blocks, median ms per call and the blocks' range; x = wideband / replaced route"]
    for role, mode in [LEGS[i] for i in args.legs]:  # (this process never opens the GPU: each leg is a fresh child under its own time limit)
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", role, mode, "--blocks", str(args.blocks), "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--sizes", *map(str, args.sizes), "--counts", *map(str, args.counts)]
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
