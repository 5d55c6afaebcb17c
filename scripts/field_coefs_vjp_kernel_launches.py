"""Twelve nf = 8 launches of the frequency response and of its coefficient adjoint per leg of scripts/field_coefs_vjp_bench.py's
workload, and nothing else: the program to put behind a kernel trace, which gives the sink kernels' durations without the upload of
the cotangents that the adjoint's launch includes.  profiles/field_coefs_vjp_kernel_trace.txt is the kernel statistics of

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o kt -- python scripts/field_coefs_vjp_kernel_launches.py
"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import random_scene
from differt2d_amd import _lib as L
from differt2d_amd.engine import Context, make_params
F = np.float32
fixed, walls = random_scene(50, seed=1234)
x = np.linspace(0.0, 1.0, 1024).astype(F)
X, Y = np.meshgrid(x, x)
inv = ((F(1) / F(0.05)) * (F(1) + np.arange(8, dtype=F) / F(64))).astype(F)
rng = np.random.default_rng(4321)
coef = (0.2 + 0.7 * rng.random(50)).astype(F)
coef[7], coef[19] = 0.0, -coef[19]
rb = rng.standard_normal((8, 1024, 1024), dtype=F); ib = rng.standard_normal((8, 1024, 1024), dtype=F)
with Context(0) as c:
    c.set_scene(walls); c.set_reflection_coefs(coef); c.set_grid(X, Y)
    for role in ("rx", "tx"):
        for mode in ("hard", "hard_sigmoid"):
            p = make_params(min_order=0, max_order=2, fun="received_power_per_object", height=0.25, approx=mode != "hard",
                            function="hard_sigmoid", grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)
            for _ in range(12):
                c.launch_frequency_response(p, fixed, inv, "sqrt")
                c.launch_field_coefs_vjp(p, fixed, inv, rb, ib, "sqrt")
            c.synchronize()
print("done")
