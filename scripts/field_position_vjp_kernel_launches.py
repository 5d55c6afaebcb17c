"""Twelve nf = 8 launches of the frequency response, of its coefficient adjoint and of its position adjoint per grid role of
scripts/field_position_vjp_bench.py's workload (hard validity), and nothing else: the program to put behind a kernel trace, which
gives the sink kernels' durations without the upload of the cotangents that both adjoints' launches include.
profiles/field_position_vjp_kernel_trace.txt is the kernel statistics of

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o kt -- python scripts/field_position_vjp_kernel_launches.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from differt2d_amd import _lib as L  # noqa: E402
from differt2d_amd.engine import Context, make_params  # noqa: E402
from field_position_vjp_bench import workload  # noqa: E402

fixed, walls, X, Y, inv, coef, rb, ib = workload(8)
with Context(0) as c:
    c.set_scene(walls)
    c.set_reflection_coefs(coef)
    c.set_grid(X, Y)
    for role in ("rx", "tx"):
        p = make_params(min_order=0, max_order=2, fun="received_power_per_object", height=0.25, approx=False,
                        grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)
        for _ in range(12):
            c.launch_frequency_response(p, fixed, inv, "sqrt")
            c.launch_field_coefs_vjp(p, fixed, inv, rb, ib, "sqrt")
            c.launch_field_position_vjp(p, fixed, inv, rb, ib, "sqrt")
        c.synchronize()
print("done")
