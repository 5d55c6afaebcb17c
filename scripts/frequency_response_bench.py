"""What does the channel frequency response cost?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024 cells, orders 0..2),
received_power, sqrt amplitudes, inv_j = (1 / 0.05) * (1 + j / 64).  Per leg (grid role x validity), on ONE context in ONE process and
one run: d2d_frequency_response_launch (power_sink_kernel with a FreqSink, one pass per 8 wavelengths over one preparation) with nf
in {1, 8, 16, 64} beside (a) ONE d2d_coherent_field_launch and (b) nf of them, one per wavelength -- the route the new call replaces.
All are interleaved in blocks so that clock drift hits all alike: HIP events around a block of back-to-back calls, median over the
blocks of the time per call (per nf launches for (b)).  Before anything is timed, plane 0 and plane nf - 1 of every nf are held bit
for bit to (b)'s results at those wavelengths.  Every leg is a child process of its own under its own time limit; the first leg that
fails ends the run.

    python scripts/frequency_response_bench.py [--out profiles/frequency_response_bench.txt] [--blocks 4] [--steps 24] [--warmup 3]
"""

import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = [("rx", "hard"), ("rx", "hard_sigmoid"), ("tx", "hard"), ("tx", "hard_sigmoid")]
LEG_SECONDS = 240
NFS = [1, 8, 16, 64]


def leg(role, mode, blocks, steps, warmup):
    from conftest import random_scene
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context, make_params

    F = np.float32
    fixed, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    inv = ((F(1) / F(0.05)) * (F(1) + np.arange(max(NFS), dtype=F) / F(64))).astype(F)
    params = make_params(min_order=0, max_order=2, approx=mode != "hard", function="hard_sigmoid",
                         grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)

    def loop(nf):
        for j in range(nf):
            c.launch_coherent_field(params, fixed, inv[j], "sqrt")

    with Context(0) as c:
        c.set_scene(walls)
        c.set_grid(X, Y)
        run = {"single": (lambda: c.launch_coherent_field(params, fixed, inv[0], "sqrt"), steps)}
        for nf in NFS:  # (the loops of 64 launches get fewer steps: a block is then as long as the others)
            run[f"freq{nf}"] = (lambda nf=nf: c.launch_frequency_response(params, fixed, inv[:nf], "sqrt"), steps)
            run[f"loop{nf}"] = (lambda nf=nf: loop(nf), max(2, steps // nf))
        for nf in sorted(NFS, reverse=True):  # warm-up, largest first: code objects, masks, the results' buffers at their final size
            for _ in range(warmup):
                run[f"freq{nf}"][0]()
        for _ in range(warmup):
            run["single"][0]()
        c.synchronize()
        # what is timed computes what it should: the first and the last plane are the single-wavelength kernel's, bit for bit
        c.launch(params, fixed)
        fused = c.get_map()
        for nf in NFS:
            fr = c.frequency_response(params, fixed, inv[:nf], "sqrt")
            assert fr.re.shape == (nf, 1024, 1024) and np.array_equal(fr.total.view(np.uint32), fused.view(np.uint32))
            for j in sorted({0, nf - 1}):
                cf = c.coherent_field(params, fixed, inv[j], "sqrt")
                assert np.array_equal(fr.re[j].view(np.uint32), cf.re.view(np.uint32)), (nf, j)
                assert np.array_equal(fr.im[j].view(np.uint32), cf.im.view(np.uint32)) and cf.im.any(), (nf, j)
            if nf > 1:
                assert not np.array_equal(fr.re[0], fr.re[nf - 1])
            del fr
        ms = {k: [] for k in run}
        for _ in range(blocks):
            for k, (f, n) in run.items():
                c.timer_begin()
                for _ in range(n):
                    f()
                ms[k].append(c.timer_end() / n)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    cols = "   ".join(f"nf={nf}: {med[f'freq{nf}']:.4f} ms (x{med[f'freq{nf}'] / med['single']:.2f} of (a), x{med[f'freq{nf}'] / med[f'loop{nf}']:.3f} of "
                      f"(b) {med[f'loop{nf}']:.4f} ms)" for nf in NFS)
    print(f"{role} {mode:13s} (a) one coherent field {med['single']:.4f} ms   frequency response {cols}   [{blocks} blocks; {steps} calls per "
          f"block, (b) max(2, {steps} // nf) loops of nf launches; planes 0 and nf-1 equal (b) by bits]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frequency_response_bench.txt"))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--leg", nargs=2, metavar=("ROLE", "MODE"), help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg[0], args.leg[1], args.blocks, args.steps, args.warmup)
        return
    lines = [f"frequency response beside (a) one coherent-field launch and (b) nf of them: configs[1] (50 walls, 1024 x 1024, orders 0..2), "
             f"received_power, sqrt amplitudes, inv_j = 20 (1 + j / 64), one context per leg, {args.blocks} interleaved blocks, median ms per call"]
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
