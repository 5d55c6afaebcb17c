#!/usr/bin/env python3
"""What the sparse emit route costs on the bench workload (BASELINE.json configs[1]: 50 walls, 1024 x 1024 cells, orders 0..2):
number of records; kernel times of the record launch's two passes and of the paths of the records, next to the fused
fun = one sweep on the same context and to the exhaustive evaluation of the same map; the host's time in `fun` and in the
accumulation; the whole call.  Hard and hard_sigmoid validity on the RX grid, hard once more on the TX grid.

    python scripts/sparse_emit_bench.py [grid side, default 1024] > profiles/sparse_emit_bench.txt"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import workload
from differt2d_amd import _lib as L
from differt2d_amd.engine import Context, make_params
from differt2d_amd.geometry import Point
from differt2d_amd.scene import Scene

g = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
fixed, walls, X, Y = workload(grid=g)
REPS = 5
med = lambda v: float(np.median(v))
cases = [("rx", "hard", dict(approx=False)), ("rx", "hard_sigmoid", dict(approx=True)), ("tx", "hard", dict(approx=False))]

with Context(0) as ctx:
    ctx.set_scene(walls); ctx.set_grid(X, Y)
    ctx.set_option("time_kernel", 1)
    for role, mode, kw in cases:
        rid = L.GRID_RX if role == "rx" else L.GRID_TX
        p = make_params(max_order=2, fun="one", grid_role=rid, **kw)
        # the fused sweep (same culling, plus the schedule, the region lists and the cut patches)
        for _ in range(4): ctx.launch(p, fixed)
        fused = []
        for _ in range(REPS):
            ctx.launch(p, fixed); fused.append(ctx.last_kernel_ms())
        fused_map = ctx.get_map()
        # the exhaustive evaluation of the same map
        if role == "rx":
            pe = make_params(max_order=2, fun="one", grid_role=rid, strict_nan=True, **kw)
            run_ex = lambda: ctx.launch_vg(pe, fixed)
        else:
            run_ex = lambda: ctx.launch(p, fixed)
            ctx.set_option("txg_exhaustive", 1)
        run_ex(); exh = []
        for _ in range(2):
            run_ex(); exh.append(ctx.last_kernel_ms())
        ctx.set_option("txg_exhaustive", 0)
        # the record launch
        ctx.valid_paths(p, fixed)
        ms, wall = [], []
        for _ in range(REPS):
            ctx.synchronize(); t = time.perf_counter()
            rec = ctx.valid_paths(p, fixed)
            wall.append((time.perf_counter() - t) * 1e3); ms.append(ctx.valid_paths_ms())
        n = rec["cell"].size
        per_cell = np.bincount(rec["cell"], minlength=X.size)
        same = np.array_equal(per_cell.reshape(X.shape) > 0, fused_map != 0) if kw["approx"] else np.array_equal(per_cell.reshape(X.shape), fused_map)
        print(f"{role} {mode} {g}^2: {n} records ({n / X.size:.3f} per cell, max {per_cell.max()}); per-cell counts equal the fused map's: {same}")
        print(f"   kernel ms (median of {REPS}): pass 1 (count) {med([m['count_ms'] for m in ms]):.3f}   pass 2 (write) {med([m['write_ms'] for m in ms]):.3f}"
              f"   paths of the records {med([m['trace_ms'] for m in ms]):.3f}")
        print(f"   fused fun=one sweep kernel {med(fused):.3f} ms   exhaustive kernel {med(exh):.3f} ms")
        print(f"   Context.valid_paths, whole call (two passes, host scan, paths, copies to host): {med(wall):.2f} ms", flush=True)

# the whole sweep through Scene, with the host's share
spent = {"fun": 0.0, "calls": 0}
def gain_fun(transmitter, receiver, path, interacting_objects, r_coef=0.5, height=0.1):
    t = time.perf_counter()
    r = path.length()
    out = (r_coef ** (path.xys.shape[-2] - 2)) / (height * height + r * r)
    spent["fun"] += time.perf_counter() - t; spent["calls"] += 1
    return out
gain_fun._d2d_native = False
import differt2d_amd.scene as S
acc_time = {"t": 0.0}
_acc = S._accumulate_sparse
def timed_acc(*a, **k):
    t = time.perf_counter(); out = _acc(*a, **k); acc_time["t"] += time.perf_counter() - t
    return out
S._accumulate_sparse = timed_acc
for role, mode, kw in cases:
    scene = Scene.from_walls_array(walls)
    if role == "rx":
        scene = scene.with_transmitters(tx=Point(xy=fixed)); sweep = scene.accumulate_on_receivers_grid_over_paths
    else:
        scene = scene.with_receivers(rx=Point(xy=fixed)); sweep = scene.accumulate_on_transmitters_grid_over_paths
    sweep(X, Y, fun=gain_fun, reduce_all=True, max_order=2, **kw)
    whole = []
    for _ in range(3):
        spent.update(fun=0.0, calls=0); acc_time["t"] = 0.0
        t = time.perf_counter(); Z = sweep(X, Y, fun=gain_fun, reduce_all=True, max_order=2, **kw); whole.append((time.perf_counter() - t) * 1e3)
    print(f"{role} {mode} {g}^2 Scene sweep with a host fun: whole call {med(whole):.1f} ms, of which the accumulation {acc_time['t'] * 1e3:.1f} ms "
          f"(in fun itself {spent['fun'] * 1e3:.1f} ms over {spent['calls']} calls); {np.count_nonzero(Z)} non-zero cells", flush=True)
