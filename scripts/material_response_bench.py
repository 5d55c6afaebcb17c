"""What does the material response cost?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024 cells, orders 0..2), TE, sqrt
amplitudes, inv_j = 20 (1 + j / 64), lossy permittivities that differ per wall.  Per leg (grid role x validity), on ONE context in ONE
process and one run, with nf in {1, 8, 64}: d2d_material_response_launch (power_sink_kernel with a MaterialSink, one pass per 8
wavelengths over one preparation) with (rows) one permittivity row per wavelength and (band) one row for the whole band, beside
(freq) the d2d_frequency_response_launch of received_power_per_object with equal nf -- what a user has today for constant real
coefficients.  All are interleaved in blocks so that clock drift hits all alike: HIP events around a block of back-to-back calls,
median over the blocks of the time per call.  Before anything is timed, the total of every material launch is held bit for bit to the
fused map of its path function, the constant band to a per-row table whose last row alone differs, and the line of sight (max_order =
0) to the frequency response.  Every leg is a child process of its own under its own time limit; the first leg that fails ends the run.

    python scripts/material_response_bench.py [--out profiles/material_response_bench.txt] [--blocks 4] [--steps 12] [--warmup 2]
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
    inv = (F(20) * (F(1) + np.arange(max(NFS), dtype=F) / F(64))).astype(F)
    f, w = np.arange(max(NFS))[:, None], np.arange(n)[None, :]
    eps = ((2.5 + 0.1 * w + 0.01 * f) - 1j * (0.05 + 0.02 * w + 0.002 * f)).astype(np.complex64)
    common = dict(min_order=0, max_order=2, approx=mode != "hard", function="hard_sigmoid", grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)
    plain = make_params(r_coef=1.0, **common)  # no reflection loss of its own: the walls' is the coefficients'
    per_object = make_params(fun="received_power_per_object", **common)
    los = make_params(r_coef=1.0, **dict(common, max_order=0))
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)

    with Context(0) as c:
        c.set_scene(walls)
        c.set_reflection_coefs(np.linspace(0.3, 0.9, n).astype(F))
        c.set_grid(X, Y)
        run = {}
        for nf in NFS:
            run[f"rows{nf}"] = (lambda nf=nf: c.launch_material_response(plain, fixed, inv[:nf], eps[:nf], "te", "sqrt"), steps)
            run[f"band{nf}"] = (lambda nf=nf: c.launch_material_response(plain, fixed, inv[:nf], eps[0], "te", "sqrt"), steps)
            run[f"freq{nf}"] = (lambda nf=nf: c.launch_frequency_response(per_object, fixed, inv[:nf], "sqrt"), steps)
        for nf in sorted(NFS, reverse=True):  # warm-up, largest first: code objects, masks, the results' buffers at their final size
            for _ in range(warmup):
                for k in ("rows", "band", "freq"):
                    run[f"{k}{nf}"][0]()
        c.synchronize()
        # what is timed computes what it should
        c.launch(plain, fixed)
        fused = c.get_map()
        assert np.isfinite(fused).all() and fused.any()
        for nf in NFS:
            rows = c.material_response(plain, fixed, inv[:nf], eps[:nf], "te", "sqrt")
            assert rows.re.shape == (nf, 1024, 1024) and np.array_equal(bits(rows.total), bits(fused)) and rows.im.any()
            band = c.material_response(plain, fixed, inv[:nf], eps[0], "te", "sqrt")
            assert np.array_equal(bits(band.total), bits(fused))
            assert np.array_equal(bits(band.re[0]), bits(rows.re[0])) and np.array_equal(bits(band.im[0]), bits(rows.im[0]))
            if nf > 1:
                assert not np.array_equal(rows.re[nf - 1], band.re[nf - 1])
                table = np.tile(eps[0], (nf, 1))
                table[-1] = eps[1]  # not constant: the per-row path over the same values
                mixed = c.material_response(plain, fixed, inv[:nf], table, "te", "sqrt")
                assert np.array_equal(bits(mixed.re[:-1]), bits(band.re[:-1])) and np.array_equal(bits(mixed.im[:-1]), bits(band.im[:-1]))
                del mixed
            del rows, band
        a = c.material_response(los, fixed, inv[:8], eps[:8], "te", "sqrt")
        b = c.frequency_response(los, fixed, inv[:8], "sqrt")
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b)) and b.im.any()
        del a, b
        ms = {k: [] for k in run}
        for _ in range(blocks):
            for k, (fn, reps) in run.items():
                c.timer_begin()
                for _ in range(reps):
                    fn()
                ms[k].append(c.timer_end() / reps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    cols = "   ".join(f"nf={nf}: rows {med[f'rows{nf}']:.4f} ms, band {med[f'band{nf}']:.4f} ms (x{med[f'band{nf}'] / med[f'rows{nf}']:.3f} of rows), "
                      f"freq {med[f'freq{nf}']:.4f} ms (rows x{med[f'rows{nf}'] / med[f'freq{nf}']:.2f}, band x{med[f'band{nf}'] / med[f'freq{nf}']:.2f} of it)"
                      for nf in NFS)
    print(f"{role} {mode:13s} {cols}   [{blocks} blocks; {steps} calls per block; totals equal the fused map, the band equals per-row tables of "
          f"equal rows and the line of sight the frequency response, by bits]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "material_response_bench.txt"))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg", nargs=2, metavar=("ROLE", "MODE"), help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg[0], args.leg[1], args.blocks, args.steps, args.warmup)
        return
    lines = [f"material response (TE; rows: a permittivity row per wavelength, band: one row for the band) beside (freq) the frequency response "
             f"of received_power_per_object with equal nf: configs[1] (50 walls, 1024 x 1024, orders 0..2), sqrt amplitudes, inv_j = 20 (1 + j / 64), "
             f"one context per leg, {args.blocks} interleaved blocks, median ms per call"]
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
