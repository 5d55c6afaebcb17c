"""What does received_power_per_object cost beside received_power?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024
cells, orders 0..2), both functions on ONE context in ONE run, interleaved in blocks so that clock and pool drift hit both alike:
forward (hard, hard_sigmoid) and value+grad with the scene VJP (hard_sigmoid).  Per leg: the median over the blocks of the
per-launch time (HIP events around a block of back-to-back launches), and the ratio of the two medians.

    python scripts/object_coefs_bench.py [--out profiles/object_coefs_bench.txt] [--blocks 7] [--steps 50]
"""

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_coefs_bench.txt"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()

    from conftest import random_scene
    from differt2d_amd.engine import Context, make_params

    F = np.float32
    tx, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    coef = (0.2 + 0.7 * np.random.default_rng(50).random(50)).astype(F)
    lines = ["received_power_per_object beside received_power: configs[1] (50 walls, 1024 x 1024, orders 0..2), one context, "
             f"{args.blocks} interleaved blocks of {args.steps} launches, median ms per launch"]
    with Context(0) as c:
        c.set_scene(walls)
        c.set_reflection_coefs(coef)
        c.set_grid(X, Y)
        c.set_cotangent(None)
        legs = [("forward hard", dict(approx=False), False, args.steps),
                ("forward hard_sigmoid", dict(approx=True), False, args.steps),
                ("value+grad+vjp hard_sigmoid", dict(approx=True), True, max(1, args.steps // 5))]
        for name, kw, vg, steps in legs:
            params = {f: make_params(fun=f, min_order=0, max_order=2, **kw) for f in ("received_power", "received_power_per_object")}
            run = (lambda p: c.launch_vg(p, tx, scene_vjp=True)) if vg else (lambda p: c.launch(p, tx))
            for p in params.values():  # warm-up: work history, masks, lists
                for _ in range(5):
                    run(p)
            c.synchronize()
            ms = {f: [] for f in params}
            for _ in range(args.blocks):
                for f, p in params.items():
                    c.timer_begin()
                    for _ in range(steps):
                        run(p)
                    ms[f].append(c.timer_end() / steps)
            a, b = float(np.median(ms["received_power"])), float(np.median(ms["received_power_per_object"]))
            lines.append(f"{name:30s} received_power {a:.4f} ms   per_object {b:.4f} ms   ratio {b / a:.3f}   "
                         f"(min {min(ms['received_power']):.4f} / {min(ms['received_power_per_object']):.4f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
