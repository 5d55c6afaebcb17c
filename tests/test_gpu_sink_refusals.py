"""The refusals of the eight products of the sink kernel, pinned to a recording: for a fixed list of refused calls in a fixed
order -- launches whose arguments break two rules at once, so that the ORDER of the checks decides the message, and getters
without a result -- the status, the full ``d2d_last_error()`` text and whether the previously accepted result is still
readable afterwards (the products discard it at different points of a refused launch) equal tests/golden/sink_refusals.json.

The fixture is a recording of the library, not a derivation: ``python tests/test_gpu_sink_refusals.py --record`` rewrites it
from whatever library ``D2D_LIB`` names, and it is only ever recorded from the commit BEFORE a change to the host launch path.
No call here gets as far as its memory check's refusal (the only message that holds a measured number), and every refusal is
decided before anything is enqueued; the accepted launches in between run on a 16 x 24 grid."""

import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "sink_refusals.json")
F = np.float32
M, N = 24, 16  # rows, columns: 3 x 2 patches
VP, I32, F32 = C.c_void_p, C.c_int32, C.c_float


def _ptr(a):
    return None if a is None else a.ctypes.data_as(VP)


class _Product:
    """One product at the C ABI: ``tail`` are the launch's arguments after (ctx, params, fixed), ``good`` a tail that is accepted,
    ``bad`` names tails that the product's own parameter check refuses, ``outs`` the getter's buffers for the good launch."""

    def __init__(self, lib, name, getter, tail, good, bad, outs, get_head=(), get_head_types=()):
        self.name, self.good, self.bad, self.outs, self.get_head = name, good, bad, outs, tuple(get_head)
        self.launch_fn = getattr(lib, f"d2d_{name}_launch")
        self.launch_fn.restype = C.c_int
        self.launch_fn.argtypes = [VP, VP, VP] + list(tail)
        self.get_fn = getattr(lib, f"d2d_get_{getter}")
        self.get_fn.restype = C.c_int
        self.get_fn.argtypes = [VP] + list(get_head_types) + [VP] * len(outs)

    def launch(self, ctx, params, fixed, tail=None):
        tail = self.good if tail is None else tail
        return self.launch_fn(ctx, None if params is None else C.addressof(params), _ptr(fixed),
                              *(_ptr(a) if isinstance(a, np.ndarray) or a is None else a for a in tail))

    def get(self, ctx, head=None, outs=None):
        outs = self.outs if outs is None else outs
        return self.get_fn(ctx, *(self.get_head if head is None else head), *(_ptr(a) for a in outs))


def _products(lib):
    cells = M * N
    inv3 = np.array([0.0, 2.5, 7.0], F)
    bad_inv3 = np.array([1.0, -2.0, 3.0], F)
    tx2 = np.array([[0.0, 0.0], [0.02, 0.0]], F)
    rx1 = np.array([[0.0, 0.0]], F)
    nan_rx1 = np.array([[0.0, np.nan]], F)
    bar = np.ones(3 * cells, F)
    f = lambda n: np.empty(n, F)
    i = lambda n: np.empty(n, np.int32)
    return [
        _Product(lib, "power_profile", "power_profile", [F32, F32, I32], (0.0, 3.0, 5),
                 {"nbins=0": (0.0, 3.0, 0), "r_max<r_min": (2.0, 1.0, 5), "r_min=inf": (float("inf"), 3.0, 5)}, [f(5 * cells)]),
        _Product(lib, "strongest_paths", "strongest_paths", [I32], (3,), {"k=0": (0,), "k=9": (9,)},
                 [f(3 * cells), f(3 * cells), i(12 * cells), i(3 * cells), f(cells), i(cells)]),
        _Product(lib, "coherent_field", "coherent_field", [F32, I32], (2.5, 0),
                 {"inv=-1": (-1.0, 0), "inv=nan": (float("nan"), 0), "amplitude=7": (2.5, 7), "inv=-1,amplitude=7": (-1.0, 7)},
                 [f(cells), f(cells), f(cells)]),
        _Product(lib, "frequency_response", "frequency_response", [VP, I32, I32], (inv3, 3, 0),
                 {"nf=0": (inv3, 0, 0), "nf=1025": (inv3, 1025, 0), "inv[1]=-2": (bad_inv3, 3, 0), "amplitude=7": (inv3, 3, 7),
                  "inv=NULL": (None, 3, 0)},
                 [f(3 * cells), f(3 * cells), f(cells)]),
        _Product(lib, "field_coefs_vjp", "field_coefs_vjp", [VP, I32, I32, VP, VP], (inv3, 3, 0, bar, bar),
                 {"nf=0": (inv3, 0, 0, bar, bar), "inv[1]=-2": (bad_inv3, 3, 0, bar, bar), "amplitude=7": (inv3, 3, 7, bar, bar),
                  "re_bar=NULL": (inv3, 3, 0, None, bar)},
                 [np.empty(7, np.float64)]),
        _Product(lib, "power_angle", "power_angle", [I32, F32, I32], (1, 0.25, 6),
                 {"end=2": (2, 0.25, 6), "origin=1": (1, 1.0, 6), "origin=nan": (1, float("nan"), 6), "nbins=4097": (1, 0.25, 4097),
                  "end=2,nbins=0": (2, 0.25, 0)},
                 [f(6 * cells), f(cells)]),
        _Product(lib, "array_response", "array_response", [F32, I32, I32, VP, I32, VP], (2.5, 0, 2, tx2, 1, rx1),
                 {"nt=0": (2.5, 0, 0, tx2, 1, rx1), "nr=9": (2.5, 0, 2, tx2, 9, rx1), "rx_elems nan": (2.5, 0, 2, tx2, 1, nan_rx1),
                  "inv=-1": (-1.0, 0, 2, tx2, 1, rx1), "amplitude=7": (2.5, 7, 2, tx2, 1, rx1), "nt=0,inv=-1": (-1.0, 0, 0, tx2, 1, rx1),
                  "tx_elems=NULL": (2.5, 0, 2, None, 1, rx1)},
                 [f(2 * cells), f(2 * cells), f(cells)]),
        _Product(lib, "array_frequency_response", "array_frequency_response", [VP, I32, I32, I32, VP, I32, VP], (inv3, 3, 0, 2, tx2, 1, rx1),
                 {"nf=0": (inv3, 0, 0, 2, tx2, 1, rx1), "inv[1]=-2": (bad_inv3, 3, 0, 2, tx2, 1, rx1), "amplitude=7": (inv3, 3, 7, 2, tx2, 1, rx1),
                  "nt=9": (inv3, 3, 0, 9, tx2, 1, rx1), "rx_elems nan": (inv3, 3, 0, 2, tx2, 1, nan_rx1), "nf=0,nt=9": (inv3, 0, 0, 9, tx2, 1, rx1),
                  "rx_elems=NULL": (inv3, 3, 0, 2, tx2, 1, None)},
                 [f(6 * cells), f(6 * cells), f(cells)], get_head=(0, 3), get_head_types=(I32, I32)),
    ]


def run_calls():
    """Issues the calls and returns their record: a list of {"product", "call", "status", "error", "readable"} in call order."""
    from conftest import random_scene, unit_grid
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context, make_params

    lib = C.CDLL(L.LIB_PATH)  # (a handle of its own on the library the package loaded: these prototypes take NULLs)
    lib.d2d_last_error.restype = C.c_char_p
    products = _products(lib)
    fixed, walls = random_scene(7, seed=77)
    X, Y = unit_grid(N, M)
    X2, Y2 = unit_grid(N - 1, M)
    coefs = np.array([0.3, 0.4, -0.7, 0.6, 0.7, 0.5, 0.0], F)
    log = []

    def base(prod, **kw):
        kw.setdefault("fun", "received_power_per_object" if prod.name == "field_coefs_vjp" else "received_power")
        return make_params(min_order=0, max_order=2, height=0.25, **kw)

    def note(prod, call, status, readable=None):
        error = lib.d2d_last_error().decode("utf-8", "replace") if status else ""
        log.append({"product": prod.name, "call": call, "status": int(status), "error": error,
                    "readable": None if readable is None else readable() == 0})

    with Context(0) as c:
        ctx = c._ctx
        for prod in products:
            note(prod, "launch without a context", prod.launch(None, base(prod), fixed))
            note(prod, "launch without a scene", prod.launch(ctx, base(prod), fixed))
            note(prod, "launch without a scene, fixed NULL, max_order 9", prod.launch(ctx, base(prod, order=9), None))
            note(prod, "get without a context", prod.get(None))
            note(prod, "get without a grid", prod.get(ctx))
        c.set_scene(walls)
        c.set_reflection_coefs(coefs)
        for prod in products:
            note(prod, "launch without a grid, solver MinPath", prod.launch(ctx, base(prod, solver="min"), fixed))
            note(prod, "launch without a grid, max_order 9", prod.launch(ctx, base(prod, order=9), fixed))
        c.set_grid(X, Y)
        for prod in products:
            note(prod, "get before any launch", prod.get(ctx))
            note(prod, "get before any launch, buffers NULL", prod.get(ctx, outs=[None] * len(prod.outs)))

        for prod in products:
            def refused(call, params, tail=None, fixed_=fixed, with_coefs=True):
                # a fresh accepted result in front of every refused call: is it still there afterwards?
                assert prod.launch(ctx, base(prod), fixed) == 0, lib.d2d_last_error()
                assert prod.get(ctx) == 0, lib.d2d_last_error()
                if not with_coefs:
                    c.set_reflection_coefs(None)
                note(prod, call, prod.launch(ctx, params, fixed_, tail), lambda: prod.get(ctx))
                if not with_coefs:
                    c.set_reflection_coefs(coefs)

            a_bad = next(iter(prod.bad))
            refused("params NULL", None)
            refused("fixed NULL, max_order 9", base(prod, order=9), fixed_=None)
            refused("max_order 9, solver MinPath", base(prod, order=9, solver="min"))
            refused("bad out_mode, " + a_bad, base(prod, out_mode=5), prod.bad[a_bad])
            refused("solver MinPath, " + a_bad, base(prod, solver="min"), prod.bad[a_bad])
            refused("solver FermatPath, sigmoid", base(prod, solver="fermat", approx=True, function="sigmoid"))
            refused("fun custom, OUT_ADD", base(prod, fun="custom", out_mode=L.OUT_ADD))
            refused("fun custom, solver MinPath", base(prod, fun="custom", solver="min"))
            refused("fun received_power, solver MinPath", base(prod, fun="received_power", solver="min"))
            refused("fun length, OUT_ADD, sigmoid", base(prod, fun="length", out_mode=L.OUT_ADD, approx=True, function="sigmoid"))
            refused("sigmoid, OUT_ADD", base(prod, out_mode=L.OUT_ADD, approx=True, function="sigmoid"))
            refused("OUT_ADD, " + a_bad, base(prod, out_mode=L.OUT_ADD), prod.bad[a_bad])
            refused("per-object coefficients missing, " + a_bad, base(prod, fun="received_power_per_object"), prod.bad[a_bad], with_coefs=False)
            refused("per-object coefficients missing, OUT_ADD", base(prod, fun="received_power_per_object", out_mode=L.OUT_ADD), with_coefs=False)
            c.set_option("txg_exhaustive", 1)
            for what, tail in prod.bad.items():
                refused(what + ", TX grid not culled", base(prod, grid_role=L.GRID_TX), tail)
            refused("sigmoid, TX grid not culled", base(prod, grid_role=L.GRID_TX, approx=True, function="sigmoid"))
            refused("TX grid not culled", base(prod, grid_role=L.GRID_TX))
            c.set_option("txg_exhaustive", 0)
            refused("TX grid, a degenerate path not exactly invalid", base(prod, grid_role=L.GRID_TX, tol=0.75))
            refused("sigmoid", base(prod, approx=True, function="sigmoid"))
            refused("sigmoid, alpha 0", base(prod, approx=True, function="sigmoid", alpha=0.0))
            if prod.name == "field_coefs_vjp":
                assert prod.launch(ctx, base(prod), fixed) == 0
                note(prod, "get with coef_bar NULL", prod.get(ctx, outs=[None]), lambda: prod.get(ctx))
            if prod.name == "array_frequency_response":
                assert prod.launch(ctx, base(prod), fixed) == 0
                for head in [(-1, 1), (0, 0), (2, 2), (3, 1)]:
                    note(prod, f"get with first {head[0]} and count {head[1]}", prod.get(ctx, head=head), lambda: prod.get(ctx))

        # every result goes with the grid ...
        for prod in products:
            assert prod.launch(ctx, base(prod), fixed) == 0, lib.d2d_last_error()
        for prod in products:
            note(prod, "get after its launch", prod.get(ctx))
        c.set_grid(X2, Y2)
        for prod in products:
            note(prod, "get after set_grid with a new grid", prod.get(ctx))
        # ... and the coefficient adjoint's with the scene as well
        c.set_grid(X, Y)
        vjp = next(p for p in products if p.name == "field_coefs_vjp")
        assert vjp.launch(ctx, base(vjp), fixed) == 0, lib.d2d_last_error()
        c.set_scene(walls[::-1].copy())
        note(vjp, "get after set_scene with another scene", vjp.get(ctx))
    return log


@pytest.fixture(scope="module")
def calls():
    return run_calls()


@pytest.mark.gpu
def test_every_refusal_equals_the_recording(calls):
    with open(FIXTURE) as fh:
        want = json.load(fh)["calls"]
    assert [(r["product"], r["call"]) for r in calls] == [(r["product"], r["call"]) for r in want]
    for got, rec in zip(calls, want):
        print(got)
        assert got == rec


@pytest.mark.gpu
def test_the_recording_covers_what_it_is_for(calls):
    """Eight products, about fifteen refused launches each or more; both discard rules occur; no measured number in any text."""
    by = {}
    for r in calls:
        by.setdefault(r["product"], []).append(r)
    assert len(by) == 8
    for name, rows in by.items():
        assert sum(1 for r in rows if r["status"] != 0 and r["readable"] is not None) >= 15, name
        assert not any("bytes free" in r["error"] for r in rows), name
    kept = {name: {r["readable"] for r in rows if r["status"] != 0 and r["readable"] is not None} for name, rows in by.items()}
    assert any(v == {True} for v in kept.values()) and any(False in v for v in kept.values())


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_sink_refusals.py --record [commit the library was built from]")
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    out = {"recorded_from": sys.argv[2] if len(sys.argv) > 2 else "unknown", "calls": run_calls()}
    with open(os.environ.get("D2D_REFUSALS_OUT", FIXTURE), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(f"{len(out['calls'])} calls recorded")
