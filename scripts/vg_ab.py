#!/usr/bin/env python3
"""A/B of the value+grad step at cfg3 (GPU box): the NaN scan beside the sweep on a stream of its own, or no scan, both grid
roles, hard and hard_sigmoid.
usage: python scripts/vg_ab.py [steps]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import workload  # noqa: E402
from differt2d_amd import _lib as L  # noqa: E402
from differt2d_amd.engine import Context, make_params  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
tx, walls, X, Y = workload()
with Context(0) as ctx:
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    for role in (L.GRID_RX, L.GRID_TX):
        for mode in (dict(approx=False), dict(approx=True), dict(approx=True, function="sigmoid")):
            p = make_params(min_order=0, max_order=2, grid_role=role, **mode)
            n = steps if mode.get("function") != "sigmoid" else max(3, steps // 10)
            for label, scan in (("beside", 1), ("no scan", 0)):
                ctx.set_option("nan_scan", scan)
                for _ in range(3):
                    ctx.launch_vg(p, tx, scene_vjp=True)
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    ctx.launch_vg(p, tx, scene_vjp=True)
                ctx.synchronize()
                ms = (time.perf_counter() - t0) / n * 1e3
                print(f"{'TX' if role == L.GRID_TX else 'RX'} grid {mode}: {label:8s} {ms:7.3f} ms per step", flush=True)
    ctx.set_option("nan_scan", 1)
