"""What does the wall adjoint of the frequency response cost?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024 cells, orders
0..2), hard validity, received_power_per_object with seeded coefficients (so that all four products run the same path function), sqrt
amplitudes, inv_j = (1 / 0.05) * (1 + j / 64), seeded standard-normal cotangents.  Per grid role, on ONE context in ONE process and one
run, with nf in {1, 8, 64}: d2d_field_walls_vjp_launch (power_sink_kernel with a WallGradSink, one pass per 8 wavelengths over one
preparation, then the fixed-order reduction of the per-patch rows) beside d2d_field_position_vjp_launch, d2d_field_coefs_vjp_launch and
d2d_frequency_response_launch of the same nf and cotangents.  The comparison is against those existing launches, never against the
new code itself.

  launch   HIP events around a block of back-to-back launches.  The three adjoints' launches include the upload of their cotangent
           planes (8 nf bytes per cell of host memory, copied before the call returns); the forward launch moves nothing.
  call     wall clock around synchronous whole calls: Context.field_walls_vjp uploads 8 nf bytes per cell and downloads 48 bytes per
           wall; Context.frequency_response downloads 8 nf + 4 bytes per cell.
  --trace  one leg's nf = 8 launches alone, four times each after a warm-up, for a kernel trace in a run of its own
           (rocprofv3 --kernel-trace --stats -- python scripts/field_walls_vjp_bench.py --trace rx).

All are interleaved in blocks so that clock drift hits all alike; medians over the blocks.  Before anything is timed, the result of
every nf is held to the bits of its own second launch.  Every leg is a child process of its own under its own time limit; the first
leg that fails ends the run.

    python scripts/field_walls_vjp_bench.py [--out profiles/field_walls_vjp_bench.txt] [--blocks 4] [--steps 12] [--warmup 2]
"""

import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = ["rx", "tx"]
LEG_SECONDS = 420
NFS = [1, 8, 64]
KINDS = ("freq", "coef", "pos", "wall")


def workload(nf_max):
    from conftest import random_scene

    F = np.float32
    fixed, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    inv = ((F(1) / F(0.05)) * (F(1) + np.arange(nf_max, dtype=F) / F(64))).astype(F)
    rng = np.random.default_rng(4321)
    coef = (0.2 + 0.7 * rng.random(50)).astype(F)
    coef[7], coef[19] = 0.0, -coef[19]
    rb = rng.standard_normal((nf_max, 1024, 1024), dtype=F)
    ib = rng.standard_normal((nf_max, 1024, 1024), dtype=F)
    return fixed, walls, X, Y, inv, coef, rb, ib


def launches(c, params, fixed, inv, rb, ib, nfs):
    launch = {}
    for nf in nfs:
        launch[f"freq{nf}"] = lambda nf=nf: c.launch_frequency_response(params, fixed, inv[:nf], "sqrt")
        launch[f"coef{nf}"] = lambda nf=nf: c.launch_field_coefs_vjp(params, fixed, inv[:nf], rb[:nf], ib[:nf], "sqrt")
        launch[f"pos{nf}"] = lambda nf=nf: c.launch_field_position_vjp(params, fixed, inv[:nf], rb[:nf], ib[:nf], "sqrt")
        launch[f"wall{nf}"] = lambda nf=nf: c.launch_field_walls_vjp(params, fixed, inv[:nf], rb[:nf], ib[:nf], "sqrt")
    return launch


def context(role, nf_max):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context, make_params

    fixed, walls, X, Y, inv, coef, rb, ib = workload(nf_max)
    params = make_params(min_order=0, max_order=2, fun="received_power_per_object", height=0.25, approx=False,
                         grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)
    c = Context(0)
    c.set_scene(walls)
    c.set_reflection_coefs(coef)
    c.set_grid(X, Y)
    return c, params, fixed, inv, rb, ib


def trace(role):
    c, params, fixed, inv, rb, ib = context(role, 8)
    with c:
        launch = launches(c, params, fixed, inv, rb, ib, [8])
        for _ in range(2):
            for f in launch.values():
                f()
        c.synchronize()
        for _ in range(4):
            for f in launch.values():
                f()
        c.synchronize()
    print(f"trace leg {role}: 2 warm-up rounds and 4 rounds of the four nf = 8 launches", flush=True)


def leg(role, blocks, steps, warmup):
    c, params, fixed, inv, rb, ib = context(role, max(NFS))
    with c:
        launch = launches(c, params, fixed, inv, rb, ib, NFS)
        call = {}
        for nf in NFS:
            call[f"freq{nf}"] = lambda nf=nf: c.frequency_response(params, fixed, inv[:nf], "sqrt")
            call[f"wall{nf}"] = lambda nf=nf: c.field_walls_vjp(params, fixed, inv[:nf], rb[:nf], ib[:nf], "sqrt")
        for nf in sorted(NFS, reverse=True):  # warm-up, largest first: code objects, masks, the buffers at their final size
            for _ in range(warmup):
                for kind in KINDS:
                    launch[f"{kind}{nf}"]()
        c.synchronize()
        # what is timed computes what it should: every result equals its own second launch by bits and is not empty
        bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
        for nf in NFS:
            g = call[f"wall{nf}"]()
            assert g.normal_bar.shape == (50, 2) and np.isfinite(g.normal_bar).all() and np.count_nonzero(g.normal_bar) >= 4, (nf, g.normal_bar)  # (few of this scene's walls carry a bounce that reaches a cell)
            again = call[f"wall{nf}"]()
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(g, again)), nf
        ms = {k: [] for k in launch}
        wall = {k: [] for k in call}
        for _ in range(blocks):
            for k, f in launch.items():
                c.timer_begin()
                for _ in range(steps):
                    f()
                ms[k].append(c.timer_end() / steps)
            for k, f in call.items():
                n = max(2, steps // 4)
                c.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    f()
                wall[k].append((time.perf_counter() - t0) * 1e3 / n)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    wmed = {k: float(np.median(v)) for k, v in wall.items()}
    cols = "   ".join(
        f"nf={nf}: launch {med[f'wall{nf}']:.4f} ms (x{med[f'wall{nf}'] / med[f'coef{nf}']:.2f} of the coefficient adjoint's {med[f'coef{nf}']:.4f} ms, "
        f"x{med[f'wall{nf}'] / med[f'pos{nf}']:.2f} of the position adjoint's {med[f'pos{nf}']:.4f} ms, "
        f"x{med[f'wall{nf}'] / med[f'freq{nf}']:.2f} of the frequency response's {med[f'freq{nf}']:.4f} ms), call {wmed[f'wall{nf}']:.3f} ms "
        f"(x{wmed[f'wall{nf}'] / wmed[f'freq{nf}']:.2f} of {wmed[f'freq{nf}']:.3f} ms)" for nf in NFS)
    print(f"{role} hard {cols}   [{blocks} blocks; {steps} launches and max(2, {steps} // 4) calls per block; every result equal to its second "
          f"launch by bits]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_walls_vjp_bench.txt"))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg", metavar="ROLE", help="(internal) run one leg in this process")
    ap.add_argument("--trace", metavar="ROLE", help="run the nf = 8 launches of one leg alone (for a kernel trace)")
    args = ap.parse_args()
    if args.trace:
        trace(args.trace)
        return
    if args.leg:
        leg(args.leg, args.blocks, args.steps, args.warmup)
        return
    lines = [f"wall adjoint of the frequency response beside its position adjoint, its coefficient adjoint and the frequency response of the same "
             f"nf: configs[1] (50 walls, 1024 x 1024, orders 0..2), hard validity, received_power_per_object, sqrt amplitudes, inv_j = 20 (1 + j / "
             f"64), one context per leg, {args.blocks} interleaved blocks, median ms; launch = HIP events around back-to-back launches (the "
             f"adjoints' include the upload of their cotangents, 8 nf bytes per cell), call = wall clock around synchronous whole calls"]
    failed = None
    for role in LEGS:  # (this process never opens the GPU: each leg is a fresh child under its own time limit)
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", role, "--blocks", str(args.blocks), "--steps", str(args.steps),
               "--warmup", str(args.warmup)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LEG_SECONDS)
        print(done.stdout, end="", flush=True)
        lines += done.stdout.splitlines()
        if done.returncode != 0:
            failed = f"leg {role} ended with status {done.returncode}: stopping"
            lines.append(failed)
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    if failed:
        sys.exit(failed)


if __name__ == "__main__":
    main()
