"""What does the permittivity adjoint of the material response cost?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024 cells,
orders 0..2), TE, sqrt amplitudes, inv_j = 20 (1 + j / 64), lossy permittivities that differ per wall, seeded standard-normal
cotangents.  Per leg (grid role x validity), on ONE context in ONE process and one run, with nf in {1, 8, 64}:
d2d_material_eps_vjp_launch (power_sink_kernel with an EpsGradSink: per 8 wavelengths the rows zeroed, one pass and one fixed-order
reduction, over one preparation) with (rows) one permittivity row per wavelength and (band) one row for the whole band, beside

  fwd      d2d_material_response_launch of equal arguments: the forward product it differentiates;
  coef     d2d_field_coefs_vjp_launch of received_power_per_object with equal nf and the same cotangents: the adjoint that exists
           today, one wave reduction per contributing candidate where this one does up to 2 K 8.

Figures per nf, medians over interleaved blocks so that clock drift hits all alike:

  launch   HIP events around a block of back-to-back launches.  Either adjoint's launch includes the upload of its cotangent planes
           (8 nf bytes per cell of pageable host memory, copied before the call returns); the forward launch moves nothing.
  kernels  the adjoint without the upload: wall clock from the return of ONE launch (the copies are through by then, the kernels
           are in flight) to the end of synchronize, on an idle stream.  It holds the zeroing, the passes and the reductions, and a
           few microseconds of the synchronisation's own.
  call     wall clock around the synchronous whole call Context.material_eps_vjp (upload + launch + download of 16 nf N bytes).

The compared route is central differences: G is holomorphic and row f depends on row f alone, so one entry of the gradient costs two
forward calls of ONE wavelength, download included: 2 nf N calls of Context.material_response with nf = 1.  A few are timed (wall
clock) and scaled.  Before anything is timed, every adjoint result is held to the bits of its own second launch.  Every leg is a child
process of its own under its own time limit; the first leg that fails ends the run.

    python scripts/material_eps_vjp_bench.py [--out profiles/material_eps_vjp_bench.txt] [--blocks 4] [--steps 8] [--warmup 2]
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
LEG_SECONDS = 280
NFS = [1, 8, 64]


def leg(role, mode, blocks, steps, warmup):
    from conftest import random_scene
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context, make_params

    F = np.float32
    fixed, walls = random_scene(50, seed=1234)
    n = len(walls)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    top = max(NFS)
    inv = (F(20) * (F(1) + np.arange(top, dtype=F) / F(64))).astype(F)
    f, w = np.arange(top)[:, None], np.arange(n)[None, :]
    eps = ((2.5 + 0.1 * w + 0.01 * f) - 1j * (0.05 + 0.02 * w + 0.002 * f)).astype(np.complex64)
    rng = np.random.default_rng(5)
    rb, ib = rng.standard_normal((top, 1024, 1024), dtype=F), rng.standard_normal((top, 1024, 1024), dtype=F)
    common = dict(min_order=0, max_order=2, approx=mode != "hard", function="hard_sigmoid", grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)
    plain = make_params(r_coef=1.0, **common)  # no reflection loss of its own: the walls' is the coefficients'
    per_object = make_params(fun="received_power_per_object", **common)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    reps = {1: steps, 8: steps, 64: max(2, steps // 4)}  # (a launch of 64 wavelengths uploads 512 MiB)

    with Context(0) as c:
        c.set_scene(walls)
        c.set_reflection_coefs(np.linspace(0.3, 0.9, n).astype(F))
        c.set_grid(X, Y)
        run = {}
        for nf in NFS:
            run[f"rows{nf}"] = lambda nf=nf: c.launch_material_eps_vjp(plain, fixed, inv[:nf], eps[:nf], rb[:nf], ib[:nf], "te", "sqrt")
            run[f"band{nf}"] = lambda nf=nf: c.launch_material_eps_vjp(plain, fixed, inv[:nf], eps[0], rb[:nf], ib[:nf], "te", "sqrt")
            run[f"fwd{nf}"] = lambda nf=nf: c.launch_material_response(plain, fixed, inv[:nf], eps[:nf], "te", "sqrt")
            run[f"coef{nf}"] = lambda nf=nf: c.launch_field_coefs_vjp(per_object, fixed, inv[:nf], rb[:nf], ib[:nf], "sqrt")
        for nf in sorted(NFS, reverse=True):  # warm-up, largest first: code objects, masks, the results' buffers at their final size
            for _ in range(warmup):
                for k in ("rows", "band", "fwd", "coef"):
                    run[f"{k}{nf}"]()
        c.synchronize()
        # what is timed computes what it should: every result equals its own second launch by bits
        for nf in NFS:
            for table in (eps[:nf], eps[0]):
                a = c.material_eps_vjp(plain, fixed, inv[:nf], table, rb[:nf], ib[:nf], "te", "sqrt")
                b = c.material_eps_vjp(plain, fixed, inv[:nf], table, rb[:nf], ib[:nf], "te", "sqrt")
                assert a.shape == (nf, n) and a.dtype == np.complex128 and np.isfinite(a).all() and np.count_nonzero(a) >= 3 * nf, (nf, a)
                assert np.array_equal(bits(a), bits(b)), nf
        ms = {k: [] for k in run}
        kern = {f"{k}{nf}": [] for nf in NFS for k in ("rows", "band", "coef")}
        call = {f"rows{nf}": [] for nf in NFS}
        fd = []
        for _ in range(blocks):
            for k, fn in run.items():
                r = reps[int("".join(ch for ch in k if ch.isdigit()))]
                c.timer_begin()
                for _ in range(r):
                    fn()
                ms[k].append(c.timer_end() / r)
            for k in kern:  # one launch on an idle stream: from its return to the end of synchronize
                c.synchronize()
                run[k]()
                t0 = time.perf_counter()
                c.synchronize()
                kern[k].append((time.perf_counter() - t0) * 1e3)
            for nf in NFS:
                c.synchronize()
                t0 = time.perf_counter()
                c.material_eps_vjp(plain, fixed, inv[:nf], eps[:nf], rb[:nf], ib[:nf], "te", "sqrt")
                call[f"rows{nf}"].append((time.perf_counter() - t0) * 1e3)
            c.synchronize()
            t0 = time.perf_counter()
            for j in range(6):  # central differences: forward calls of one wavelength, download included
                c.material_response(plain, fixed, inv[j:j + 1], eps[j:j + 1], "te", "sqrt")
            fd.append((time.perf_counter() - t0) * 1e3 / 6)
    med = lambda v: float(np.median(v))
    one = med(fd)
    cols = []
    for nf in NFS:
        r, b, fw, co = (med(ms[f"{k}{nf}"]) for k in ("rows", "band", "fwd", "coef"))
        kr, kb, kc = (med(kern[f"{k}{nf}"]) for k in ("rows", "band", "coef"))
        cols.append(f"nf={nf}: launch rows {r:.4f} ms, band {b:.4f} ms, fwd {fw:.4f} ms, coef {co:.4f} ms; kernels (no upload) rows {kr:.4f} ms "
                    f"(x{kr / fw:.2f} of fwd, x{kr / kc:.2f} of coef's {kc:.4f}), band {kb:.4f} ms (x{kb / kr:.3f} of rows); call {med(call[f'rows{nf}']):.3f} ms; "
                    f"central differences 2 * {nf} * {n} calls of {one:.3f} ms = {2 * nf * n * one:.0f} ms (x{2 * nf * n * one / med(call[f'rows{nf}']):.0f} of the call)")
    print(f"{role} {mode:13s} " + "   ".join(cols) + f"   [{blocks} blocks; {steps} launches per block ({reps[64]} at nf=64); every result equals its "
          f"second launch by bits]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "material_eps_vjp_bench.txt"))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg", nargs=2, metavar=("ROLE", "MODE"), help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg[0], args.leg[1], args.blocks, args.steps, args.warmup)
        return
    lines = [f"permittivity adjoint of the material response (TE; rows: a permittivity row per wavelength, band: one row for the band) beside (fwd) "
             f"the material response of equal arguments and (coef) the coefficient adjoint of received_power_per_object with equal nf and cotangents: "
             f"configs[1] (50 walls, 1024 x 1024, orders 0..2), sqrt amplitudes, inv_j = 20 (1 + j / 64), one context per leg, {args.blocks} "
             f"interleaved blocks, medians; launch = HIP events around back-to-back launches (an adjoint's includes the upload of its cotangents, "
             f"8 nf bytes per cell), kernels = wall clock from one launch's return to the end of synchronize (no upload), call = wall clock of "
             f"Context.material_eps_vjp, central differences = 2 nf N forward calls of one wavelength with their downloads, 6 timed per block and scaled"]
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
