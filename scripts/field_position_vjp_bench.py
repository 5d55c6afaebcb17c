"""What does the position adjoint of the frequency response cost?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024 cells,
orders 0..2), hard validity, received_power_per_object with seeded coefficients (so that all three products run the same path
function), sqrt amplitudes, inv_j = (1 / 0.05) * (1 + j / 64), seeded standard-normal cotangents.  Per grid role, on ONE context in ONE
process and one run, with nf in {1, 8, 64}: d2d_field_position_vjp_launch (power_sink_kernel with a PosGradSink, one pass per 8
wavelengths over one preparation, then the two-stage fixed-order sum) beside d2d_frequency_response_launch (the forward product it
differentiates) and d2d_field_coefs_vjp_launch (the adjoint that holds the same cotangents in registers) of the same nf and cotangents.

  launch   HIP events around a block of back-to-back launches.  Both adjoints' launches include the upload of their cotangent planes
           (8 nf bytes per cell of host memory, copied before the call returns); the forward launch moves nothing.  The kernels
           without the upload come from a kernel trace of scripts/field_position_vjp_kernel_launches.py.
  call     wall clock around synchronous whole calls: Context.frequency_response downloads 8 nf + 4 bytes per cell,
           Context.field_position_vjp uploads 8 nf and downloads 16 bytes per cell.
  fd       the only other route to the same gradients, central differences: wall clock of four re-gridded forward calls (the grid
           displaced by +-h along x and y: d2d_set_grid and Context.frequency_response each) for cell_bar, and of four forward calls
           with the fixed end point displaced for fixed_bar -- whose fp32 result is not usable (DESIGN.md K3-X says why).

All are interleaved in blocks so that clock drift hits all alike; medians over the blocks.  Before anything is timed, the result of
every nf is held to the bits of its own second launch.  Every leg is a child process of its own under its own time limit; the first
leg that fails ends the run.

    python scripts/field_position_vjp_bench.py [--out profiles/field_position_vjp_bench.txt] [--blocks 4] [--steps 12] [--warmup 2]
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


def leg(role, blocks, steps, warmup):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context, make_params

    F = np.float32
    fixed, walls, X, Y, inv, coef, rb, ib = workload(max(NFS))
    params = make_params(min_order=0, max_order=2, fun="received_power_per_object", height=0.25, approx=False,
                         grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)
    h = F(1e-4)
    with Context(0) as c:
        c.set_scene(walls)
        c.set_reflection_coefs(coef)
        c.set_grid(X, Y)
        launch, call = {}, {}
        for nf in NFS:
            launch[f"freq{nf}"] = lambda nf=nf: c.launch_frequency_response(params, fixed, inv[:nf], "sqrt")
            launch[f"coef{nf}"] = lambda nf=nf: c.launch_field_coefs_vjp(params, fixed, inv[:nf], rb[:nf], ib[:nf], "sqrt")
            launch[f"pos{nf}"] = lambda nf=nf: c.launch_field_position_vjp(params, fixed, inv[:nf], rb[:nf], ib[:nf], "sqrt")
            call[f"freq{nf}"] = lambda nf=nf: c.frequency_response(params, fixed, inv[:nf], "sqrt")
            call[f"pos{nf}"] = lambda nf=nf: c.field_position_vjp(params, fixed, inv[:nf], rb[:nf], ib[:nf], "sqrt")
        for nf in sorted(NFS, reverse=True):  # warm-up, largest first: code objects, masks, the buffers at their final size
            for _ in range(warmup):
                for kind in ("freq", "coef", "pos"):
                    launch[f"{kind}{nf}"]()
        c.synchronize()
        # what is timed computes what it should: every result equals its own second launch by bits and is not empty
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)
        for nf in NFS:
            g = call[f"pos{nf}"]()
            assert g.cell_bar.shape == (1024, 1024, 2) and np.isfinite(g.fixed_bar).all() and g.fixed_bar.all(), (nf, g.fixed_bar)
            lit = (np.count_nonzero(g.cell_bar), np.count_nonzero(g.fixed_terms))
            assert min(lit) > 1e5, (nf, lit)  # (most cells of this scene lie in shadow of every path)
            again = call[f"pos{nf}"]()
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(g, again)), nf
            del g, again
        shifted = [((X + sx * h).astype(F), (Y + sy * h).astype(F)) for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1))]
        moved = [np.asarray(fixed, F) + np.array(d, F) * h for d in ((1, 0), (-1, 0), (0, 1), (0, -1))]

        def fd_cells(nf):
            for Xs, Ys in shifted:
                c.set_grid(Xs, Ys)
                c.frequency_response(params, fixed, inv[:nf], "sqrt")
            c.set_grid(X, Y)

        def fd_fixed(nf):
            for f2 in moved:
                c.frequency_response(params, f2, inv[:nf], "sqrt")

        ms = {k: [] for k in launch}
        wall = {k: [] for k in list(call) + [f"fdc{nf}" for nf in NFS] + [f"fdf{nf}" for nf in NFS]}
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
            for nf in NFS:
                for key, f in ((f"fdc{nf}", fd_cells), (f"fdf{nf}", fd_fixed)):
                    c.synchronize()
                    t0 = time.perf_counter()
                    f(nf)
                    wall[key].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    wmed = {k: float(np.median(v)) for k, v in wall.items()}
    cols = "   ".join(
        f"nf={nf}: launch {med[f'pos{nf}']:.4f} ms (x{med[f'pos{nf}'] / med[f'coef{nf}']:.2f} of the coefficient adjoint's {med[f'coef{nf}']:.4f} ms, "
        f"x{med[f'pos{nf}'] / med[f'freq{nf}']:.2f} of the frequency response's {med[f'freq{nf}']:.4f} ms), call {wmed[f'pos{nf}']:.3f} ms "
        f"(x{wmed[f'pos{nf}'] / wmed[f'freq{nf}']:.2f} of {wmed[f'freq{nf}']:.3f} ms), central differences {wmed[f'fdc{nf}']:.1f} ms for the cells "
        f"and {wmed[f'fdf{nf}']:.1f} ms for the fixed end" for nf in NFS)
    print(f"{role} hard {cols}   [{blocks} blocks; {steps} launches and max(2, {steps} // 4) calls per block; every result equal to its second "
          f"launch by bits]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_position_vjp_bench.txt"))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg", metavar="ROLE", help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.blocks, args.steps, args.warmup)
        return
    lines = [f"position adjoint of the frequency response beside the frequency response and its coefficient adjoint of the same nf: configs[1] "
             f"(50 walls, 1024 x 1024, orders 0..2), hard validity, received_power_per_object, sqrt amplitudes, inv_j = 20 (1 + j / 64), one "
             f"context per leg, {args.blocks} interleaved blocks, median ms; launch = HIP events around back-to-back launches (both adjoints' "
             f"include the upload of their cotangents, 8 nf bytes per cell), call = wall clock around synchronous whole calls, central "
             f"differences = wall clock of four displaced forward calls (re-gridded for the cells)"]
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
