#!/usr/bin/env python3
"""Where the record launch's time goes: the fused fun = one sweep kernel on the bench workload with its
launch options taken away one by one -- region lists, cut patches, the dearest-first schedule, the pipelined preparation --
next to the two passes of the record launch (Context.valid_paths) on the same context.

    python scripts/sparse_emit_where.py > profiles/sparse_emit_where.txt"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import workload
from differt2d_amd import _lib as L
from differt2d_amd.engine import Context, make_params
fixed, walls, X, Y = workload(grid=1024)
med = lambda v: float(np.median(v))
steps = [("default", {}), ("region_lists=0", {"region_lists": 0}), ("+ heavy_split=0", {"heavy_split": 0}),
         ("+ identity schedule (sched_min_tiles huge)", {"sched_min_tiles": 1 << 40}), ("+ pipeline=0", {"pipeline": 0})]
for role, kw in (("rx", dict(approx=False)), ("rx", dict(approx=True)), ("tx", dict(approx=False))):
    with Context(0) as ctx:
        ctx.set_scene(walls); ctx.set_grid(X, Y); ctx.set_option("time_kernel", 1)
        p = make_params(max_order=2, fun="one", grid_role=L.GRID_RX if role == "rx" else L.GRID_TX, **kw)
        for name, opts in steps:
            for k, v in opts.items(): ctx.set_option(k, v)
            for _ in range(5): ctx.launch(p, fixed)
            t = []
            for _ in range(7):
                ctx.launch(p, fixed); t.append(ctx.last_kernel_ms())
            print(f"{role} approx={kw['approx']} fused one sweep, {name}: kernel {med(t):.3f} ms  shape {ctx.sweep_shape()}", flush=True)
        ctx.valid_paths(p, fixed)
        ms = []
        for _ in range(5):
            ctx.valid_paths(p, fixed); ms.append(ctx.valid_paths_ms())
        print(f"{role} approx={kw['approx']} record launch: count {med([m['count_ms'] for m in ms]):.3f}  write {med([m['write_ms'] for m in ms]):.3f}  paths {med([m['trace_ms'] for m in ms]):.3f} ms", flush=True)
