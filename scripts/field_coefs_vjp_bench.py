"""What does the coefficient adjoint of the frequency response cost?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024 cells,
orders 0..2), received_power_per_object with seeded coefficients (one zero, one negative), sqrt amplitudes, inv_j = (1 / 0.05) *
(1 + j / 64), seeded standard-normal cotangents.  Per leg (grid role x validity), on ONE context in ONE process and one run, with nf in
{1, 8, 16, 64}: d2d_field_coefs_vjp_launch (power_sink_kernel with a CoefGradSink, one pass per 8 wavelengths over one preparation,
then the fixed-order reduction) beside d2d_frequency_response_launch of the same nf and the same path function -- the forward product
it differentiates, and the yardstick.  Two figures per nf:

  launch   HIP events around a block of back-to-back launches.  The adjoint's launch includes the upload of its cotangent planes
           (8 nf bytes per cell of host memory, copied before the call returns); the forward launch moves nothing.
  call     wall clock around synchronous whole calls, Context.frequency_response (launch + download of 8 nf + 4 bytes per cell)
           beside Context.field_coefs_vjp (upload of 8 nf bytes per cell + launch + download of N doubles): both move the same planes
           over the same bus, in opposite directions.

All are interleaved in blocks so that clock drift hits all alike; medians over the blocks.  Before anything is timed, the result of
every nf is held to the bits of its own second launch, and the first chunk's share to a launch of its own.  Every leg is a child
process of its own under its own time limit; the first leg that fails ends the run.

    python scripts/field_coefs_vjp_bench.py [--out profiles/field_coefs_vjp_bench.txt] [--blocks 4] [--steps 12] [--warmup 2]
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

LEGS = [("rx", "hard"), ("rx", "hard_sigmoid"), ("tx", "hard"), ("tx", "hard_sigmoid")]
LEG_SECONDS = 300
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
    rng = np.random.default_rng(4321)
    coef = (0.2 + 0.7 * rng.random(50)).astype(F)
    coef[7], coef[19] = 0.0, -coef[19]
    rb = rng.standard_normal((max(NFS), 1024, 1024), dtype=F)
    ib = rng.standard_normal((max(NFS), 1024, 1024), dtype=F)
    params = make_params(min_order=0, max_order=2, fun="received_power_per_object", height=0.25, approx=mode != "hard",
                         function="hard_sigmoid", grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)

    with Context(0) as c:
        c.set_scene(walls)
        c.set_reflection_coefs(coef)
        c.set_grid(X, Y)
        launch = {}
        for nf in NFS:
            launch[f"freq{nf}"] = lambda nf=nf: c.launch_frequency_response(params, fixed, inv[:nf], "sqrt")
            launch[f"vjp{nf}"] = lambda nf=nf: c.launch_field_coefs_vjp(params, fixed, inv[:nf], rb[:nf], ib[:nf], "sqrt")
        call = {}
        for nf in NFS:
            call[f"freq{nf}"] = lambda nf=nf: c.frequency_response(params, fixed, inv[:nf], "sqrt")
            call[f"vjp{nf}"] = lambda nf=nf: c.field_coefs_vjp(params, fixed, inv[:nf], rb[:nf], ib[:nf], "sqrt")
        for nf in sorted(NFS, reverse=True):  # warm-up, largest first: code objects, masks, the buffers at their final size
            for _ in range(warmup):
                launch[f"freq{nf}"]()
                launch[f"vjp{nf}"]()
        c.synchronize()
        # what is timed computes what it should: every result equals its own second launch by bits, has a gradient on the walls that
        # carry paths, and the first chunk's share of a longer list
        # is the 8-entry launch
        bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
        for nf in NFS:
            g = call[f"vjp{nf}"]()
            assert g.shape == (50,) and g.dtype == np.float64 and np.isfinite(g).all() and np.count_nonzero(g) >= 3, (nf, g)
            assert np.array_equal(bits(call[f"vjp{nf}"]()), bits(g)), nf
            if nf > 8:
                rz, iz = np.zeros_like(rb[:nf]), np.zeros_like(ib[:nf])
                rz[:8], iz[:8] = rb[:8], ib[:8]
                first = c.field_coefs_vjp(params, fixed, inv[:nf], rz, iz, "sqrt")
                assert np.array_equal(bits(first), bits(c.field_coefs_vjp(params, fixed, inv[:8], rb[:8], ib[:8], "sqrt"))), nf
                del rz, iz
        assert g[7] == 0.0 and not np.signbit(g[7])  # sqrt amplitudes: the zero coefficient's wall has no term, exactly +0.0
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
    cols = "   ".join(f"nf={nf}: launch {med[f'vjp{nf}']:.4f} ms (x{med[f'vjp{nf}'] / med[f'freq{nf}']:.2f} of the frequency response's "
                      f"{med[f'freq{nf}']:.4f} ms), call {wmed[f'vjp{nf}']:.3f} ms (x{wmed[f'vjp{nf}'] / wmed[f'freq{nf}']:.2f} of {wmed[f'freq{nf}']:.3f} ms)"
                      for nf in NFS)
    print(f"{role} {mode:13s} {cols}   [{blocks} blocks; {steps} launches and max(2, {steps} // 4) calls per block; every result equal to its "
          f"second launch by bits]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_coefs_vjp_bench.txt"))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg", nargs=2, metavar=("ROLE", "MODE"), help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg[0], args.leg[1], args.blocks, args.steps, args.warmup)
        return
    lines = [f"coefficient adjoint of the frequency response beside the frequency response of the same nf: configs[1] (50 walls, 1024 x 1024, "
             f"orders 0..2), received_power_per_object, sqrt amplitudes, inv_j = 20 (1 + j / 64), one context per leg, {args.blocks} interleaved "
             f"blocks, median ms; launch = HIP events around back-to-back launches (the adjoint's includes the upload of its cotangents, "
             f"8 nf bytes per cell), call = wall clock around synchronous whole calls (both move 8 nf bytes per cell over the bus)"]
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
