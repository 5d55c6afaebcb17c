"""What does the beam-space response cost beside the route it replaces?  BASELINE.json configs[1] (50 walls, seed 1234, 1024 x 1024
cells, orders 0..2), half-wavelength uniform linear arrays of 4 x 4 and 8 x 8 elements at nf = 8 and 64 inverse wavelengths
20 + k / 32, hard and hard_sigmoid validity, both grid roles, codebooks of 1 x 1, 1 x 8 and 8 x 8 (receive x transmit) beams of
utils.steering_weights.  Per leg, element count and wavelength count, on ONE context in ONE process, two comparisons:

  whole call    Context.beam_response (launch + get, synchronous) beside the route it replaces: Context.array_frequency_response
                (launch + get of the 2 nf nr nt element-space planes) and then utils.beamformed_power per wavelength and beam pair on
                the host.  The host share is timed on `--host-sample` (wavelength, pair) evaluations and scaled to all nf nbr nbt of them
                (0: every one is run); the line says which.  A result of more than GET_BYTES is read in ranges of wavelengths, as
                the getters allow for results larger than host memory, on both sides alike; the line says in how many.  Where the
                route's planes exceed half of the free device memory the line says that the route does not run at all.
  launch alone  launch_beam_response beside launch_array_frequency_response of the same nf, nt, nr (HIP events around a block of
                back-to-back launches).

Blocks of the two are interleaved so that clock drift hits both alike; the lines give the median over the blocks and the blocks' own
range, and whether the slowest beam block beats the fastest block of the route.  Before anything is timed, after a warm-up of every
shape, one plane of every beam result (the last wavelength, the last pair) is held to the element-space bound of
tests/beam_response_oracle.py against the float64 contraction of Context.array_frequency_response's planes (see `check`).
Every (leg, element count, wavelength count) is a child process of its own under its own time limit; the first that fails ends the
run.  One invocation with the defaults writes the whole of profiles/beam_response_bench.txt.

    python scripts/beam_response_bench.py [--out profiles/beam_response_bench.txt] [--blocks 3] [--sizes 4 8] [--counts 8 64]
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

WAVELENGTH = 0.05
SIZES = [4, 8]      # n x n elements
COUNTS = [8, 64]    # nf
BOOKS = [(1, 1), (1, 8), (8, 8)]  # nbr x nbt
LEGS = [("rx", "hard"), ("rx", "hard_sigmoid"), ("tx", "hard"), ("tx", "hard_sigmoid")]
CHILD_SECONDS = 600
GET_BYTES = 8 << 30  # re and im of one get on the host; larger results are read in ranges of wavelengths


def check(got_re, got_im, H_re, H_im, w_rx, w_tx, sum_a, count, inv, n):
    """One beam plane against the float64 contraction of the element-space planes of the same wavelength, per cell, within an UPPER
    ENVELOPE of the element-space bound of tests/beam_response_oracle.py (``bound``: its derivation is there; the oracle's own bound
    needs every contribution of every cell, which a 1024 x 1024 grid does not keep).  Every per-contribution term is taken at its
    largest, so this check is looser than the tests': ``sum_a`` is the cell's sum of amplitudes, those of contributions without a
    direction included (the coherent field at inverse wavelength 0, where every phase is 0),
    ``count`` its number of contributions (the strongest-paths build counts them), path lengths stay below 4.3 (two reflections in
    the unit square) and ``|q|`` below the array's half length."""
    y = np.einsum("i,ij...,j->...", w_rx.conj().astype(np.complex128), H_re.astype(np.float64) + 1j * H_im, w_tx.astype(np.complex128))
    e = 2.0**-24
    half = (n - 1) / 2 * WAVELENGTH / 2
    ulp = lambda x: float(np.spacing(np.float32(x)))  # noqa: E731
    turns = ulp(4.3 * inv) + ulp(half * inv) + 2.5 * ulp(2 * half * inv) + 2.5 * e
    per = 2 * np.pi * turns + (32 + 4 * n + 3 * count.astype(np.float64)) * e
    bound = (1 + 2.0**-10) * np.abs(sum_a.astype(np.float64)) * (1 + count * e) * per * np.abs(w_rx).sum() * np.abs(w_tx).sum()
    err = np.abs((got_re.astype(np.float64) + 1j * got_im) - y)
    assert (err <= bound).all(), (float(err.max()), float(bound[err > bound].min()))
    return float(np.abs(y).max()), float(err.max()), float((err[bound > 0] / bound[bound > 0]).max())


def ranges(nf, planes):
    """``(first, count)`` ranges of wavelengths whose re and im, ``planes`` plane pairs of 1024 x 1024 fp32 per wavelength, stay
    within GET_BYTES per get: one range where the whole result does."""
    per = max(1, GET_BYTES // (8 * planes * 1024 * 1024))
    return [(first, min(per, nf - first)) for first in range(0, nf, per)]


def leg(role, mode, blocks, steps, warmup, sizes, counts, host_sample):
    from conftest import random_scene
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context, make_params
    from differt2d_amd.utils import array_response_at, beamformed_power, steering_weights, ula

    F = np.float32
    fixed, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    inv = {nf: (F(20) + np.arange(nf, dtype=F) / F(32)).astype(F) for nf in counts}
    params = make_params(min_order=0, max_order=2, approx=mode != "hard", function="hard_sigmoid",
                         grid_role=L.GRID_RX if role == "rx" else L.GRID_TX)
    arrays = {n: (ula(n, WAVELENGTH / 2), ula(n, WAVELENGTH / 2, np.pi / 2)) for n in sizes}
    angles = np.linspace(0.0, np.pi, 8, endpoint=False)
    books = {(n, b): (steering_weights(arrays[n][0], angles[:b[1]] + np.pi, WAVELENGTH), steering_weights(arrays[n][1], angles[:b[0]], WAVELENGTH))
             for n in sizes for b in BOOKS}
    out = []
    with Context(0) as c:
        c.set_scene(walls)
        c.set_grid(X, Y)
        c.launch(params, fixed)
        lit = float((c.get_map() != 0).mean())
        sum_a = c.coherent_field(params, fixed, 0.0, "sqrt").re  # every phase is 0: the sum of the amplitudes
        count = c.strongest_paths(params, fixed, 1).count
        assert (sum_a >= 0).all() and count.max() >= 1
        out.append(f"{role} {mode:13s} ({100 * lit:.1f} % of the cells lit; one plane of every beam result within the element-space bound of the "
                   f"float64 contraction of Context.array_frequency_response)")
        for n in sizes:
            etx, erx = arrays[n]
            for nf in counts:
                wide = lambda: c.launch_array_frequency_response(params, fixed, inv[nf], etx, erx, "sqrt")  # noqa: E731
                route_runs = True
                try:
                    for _ in range(warmup):
                        wide()
                    c.synchronize()
                except L.D2DUnsupported as e:
                    route_runs = False
                    out.append(f"    {n} x {n}, nf = {nf}: the replaced route does not run at all ({str(e).split(': ', 1)[-1]})")
                H = c.get_array_frequency_response(nf - 1, 1) if route_runs else None
                for b in BOOKS:
                    wtx, wrx = books[(n, b)]
                    beam = lambda: c.launch_beam_response(params, fixed, inv[nf], etx, erx, wtx, wrx, "sqrt")  # noqa: E731
                    for _ in range(warmup):
                        beam()
                    c.synchronize()
                    head = f"    {n} x {n}, nf = {nf:2d}, codebook {b[0]} x {b[1]}:"
                    if route_runs:
                        got = c.get_beam_response(nf - 1, 1)
                        peak, err, ratio = check(got.re[0, -1, -1], got.im[0, -1, -1], H.re[0], H.im[0], wrx[-1], wtx[-1], sum_a, count, float(inv[nf][-1]), n)
                        head += f" [checked: max |y| {peak:.3e}, max error {err:.2e}, max error / bound {ratio:.3f}]"
                        del got
                    # launch alone: HIP events around back-to-back launches, interleaved blocks
                    reps = max(3, min(steps, steps * 64 // (nf * max(n * n, b[0] * b[1]))))
                    lb, lw = [], []
                    for _ in range(blocks):
                        c.timer_begin()
                        for _ in range(reps):
                            beam()
                        lb.append(c.timer_end() / reps)
                        if route_runs:
                            c.timer_begin()
                            for _ in range(reps):
                                wide()
                            lw.append(c.timer_end() / reps)
                    # whole call: launch + get, synchronous, wall clock; the route adds beamformed_power per wavelength and pair
                    wb, wr, host = [], [], []
                    pairs = [(f, br, bt) for f in range(nf) for br in range(b[0]) for bt in range(b[1])]
                    sample = pairs if host_sample <= 0 or host_sample >= len(pairs) else [pairs[k * len(pairs) // host_sample] for k in range(host_sample)]
                    rb, rw = ranges(nf, b[0] * b[1]), ranges(nf, n * n)
                    for _ in range(blocks):
                        t0 = time.perf_counter()
                        beam()
                        for lo, cnt in rb:
                            part = c.get_beam_response(lo, cnt, with_total=lo == 0)
                            del part
                        wb.append(1e3 * (time.perf_counter() - t0))
                        if route_runs:
                            spent = 0.0
                            t0 = time.perf_counter()
                            wide()
                            for lo, cnt in rw:
                                afr = c.get_array_frequency_response(lo, cnt, with_total=lo == 0)
                                t1 = time.perf_counter()
                                for f, br, bt in sample:
                                    if lo <= f < lo + cnt:
                                        beamformed_power(array_response_at(afr, f - lo), wrx[br], wtx[bt])
                                spent += time.perf_counter() - t1
                                del afr
                            whole = time.perf_counter() - t0
                            host.append(1e3 * spent * len(pairs) / len(sample))
                            wr.append(1e3 * (whole - spent) + host[-1])
                    span = lambda v: f"{np.median(v):10.3f} ms (blocks {min(v):.3f} .. {max(v):.3f})"  # noqa: E731
                    if route_runs:
                        scaled = "every evaluation run" if len(sample) == len(pairs) else f"{len(sample)} of {len(pairs)} evaluations run and scaled"
                        if len(rb) > 1 or len(rw) > 1:
                            scaled += f"; gets in {len(rb)} / {len(rw)} ranges of wavelengths"
                        ok = max(wb) < min(wr)
                        out.append(f"{head}\n        whole call   beam {span(wb)}   route {span(wr)} of which host {np.median(host):.1f} ms ({scaled})   "
                                   f"x{np.median(wb) / np.median(wr):.4f}   {'every block faster' if ok else 'NOT faster in every block'}"
                                   f"{'' if b[0] * b[1] <= n * n else '   (nbr nbt > nr nt: no requirement)'}\n"
                                   f"        launch alone beam {span(lb)}   array_frequency_response {span(lw)}   x{np.median(lb) / np.median(lw):.3f}   "
                                   f"[{reps} launches per block]")
                    else:
                        out.append(f"{head}\n        whole call   beam {span(wb)}   route: does not run\n        launch alone beam {span(lb)}   [{reps} launches per block]")
                    print(out[-1], flush=True)
                del H
    print("\n".join(out[:1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_response_bench.txt"))
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
    ap.add_argument("--counts", type=int, nargs="+", default=COUNTS)
    ap.add_argument("--host-sample", type=int, default=2, help="(wavelength, pair) evaluations of beamformed_power timed per block; 0: all")
    ap.add_argument("--legs", type=int, nargs="+", default=list(range(len(LEGS))), help="indices into the four legs")
    ap.add_argument("--leg", nargs=2, metavar=("ROLE", "MODE"), help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg[0], args.leg[1], args.blocks, args.steps, args.warmup, args.sizes, args.counts, args.host_sample)
        return
    lines = [f"beam-space response beside the route it replaces: configs[1] (50 walls, 1024 x 1024, orders 0..2), received_power, inverse "
             f"wavelengths 20 + k / 32, half-wavelength ULAs (transmit along x, receive along y), steering_weights codebooks (receive x transmit "
             f"beams), amplitude sqrt, one context per leg, size and count, {args.blocks} interleaved blocks, median and the blocks' range; whole call = launch + "
             f"get (+ utils.beamformed_power per wavelength and pair for the route), wall clock; launch alone by HIP events; x = beam / route"]
    # (this process never opens the GPU: each leg, size and count is a fresh child under its own time limit)
    for role, mode in [LEGS[i] for i in args.legs]:
        for n in args.sizes:
            for nf in args.counts:
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", role, mode, "--blocks", str(args.blocks), "--steps", str(args.steps),
                       "--warmup", str(args.warmup), "--sizes", str(n), "--counts", str(nf), "--host-sample", str(args.host_sample)]
                done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=CHILD_SECONDS)
                print(done.stdout, end="", flush=True)
                if done.returncode != 0:
                    sys.exit(f"{role} {mode} {n} x {n} nf = {nf} ended with status {done.returncode}: stopping")
                body = done.stdout.splitlines()
                lines += body[-1:] + body[:-1]  # (the child prints its heading last)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
