"""Kernel traces of the wideband array response, in runs of their own (tracing slows the host: nothing here is an end-to-end time).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/array_frequency_response_trace.py run ROLE MODE N NF
    python scripts/array_frequency_response_trace.py condense DIR LABEL >> profiles/array_frequency_response_kernel_trace.txt

`run` does twelve launches of one shape at BASELINE.json configs[1], 1024 x 1024 (N x N half-wavelength ULAs, NF inverse wavelengths
20 + k / 32) and nothing else; `condense` sums the trace per kernel name: share of all kernel time, total, dispatches, time per
dispatch.  __amd_rocclr_fillBufferAligned is the zeroing of the planes."""
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(role, mode, n, nf):
    from conftest import random_scene
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context, make_params
    from differt2d_amd.utils import ula

    F = np.float32
    fixed, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    inv = (F(20) + np.arange(nf, dtype=F) / F(32)).astype(F)
    params = make_params(min_order=0, max_order=2, approx=mode != "hard", function="hard_sigmoid",
                         grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)
    with Context(0) as c:
        c.set_scene(walls)
        c.set_grid(X, Y)
        for _ in range(12):
            c.launch_array_frequency_response(params, fixed, inv, ula(n, 0.025), ula(n, 0.025, np.pi / 2), "sqrt")
        c.synchronize()


def condense(d, label):
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    assert files, "no kernel trace under " + d
    tot = {}
    for fn in files:
        for row in csv.DictReader(open(fn)):
            c = tot.setdefault(row["Kernel_Name"], [0, 0])
            c[0] += 1
            c[1] += int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
    all_ns = sum(v[1] for v in tot.values())
    print(f"{label}: {sum(v[0] for v in tot.values())} dispatches, {all_ns / 1e6:.3f} ms of kernel time in all")
    for name, (calls, ns) in sorted(tot.items(), key=lambda kv: -kv[1][1]):
        short = name if len(name) <= 110 else name[:107] + "..."
        print(f"    {100 * ns / all_ns:5.1f} %  {ns / 1e6:10.3f} ms  {calls:5d} calls  {ns / calls / 1e6:9.4f} ms each  {short}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    elif sys.argv[1] == "condense":
        condense(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
