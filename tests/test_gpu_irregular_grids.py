"""The sweeps and the sink products on grids that are no axis-aligned mesh (include/d2d.h: d2d_set_grid takes "any coordinates").

Every other test of the suite builds its grid with ``np.meshgrid``, where the corner lanes of a patch and the corner cells of a region
are the extremes of their boxes, neighbouring boxes are disjoint and of positive extent, rows are monotone and no two cells coincide.
The culling is written against boxes that make none of this matter -- the shuffle reductions of ``fwd_patch`` / ``split_patch`` /
``power_fwd_coop_kernel`` / ``txg_patch`` and of the sink kernel's ``wave_prologue``, ``region_box_kernel``, ``hidden_region_kernel``'s
``bb``, the ``nan_possible_*`` tests of the NaN scan, the TX-grid chain -- and here that is checked, on the grids of
``tests/irregular_grids.py``: scene R (a room with clutter, 14 walls) on ``mesh`` (the control), ``scrambled`` (every patch's box is
nearly the whole scene), ``sheared`` (overlapping boxes), ``polar`` (two coincident rows; inner boxes contain the fixed end point),
``track_row`` / ``track_col`` (seven of eight lanes are clamped copies), ``collapsed`` (a row of patches with a box of zero extent) and
``flipped``; the lattice scenes L3, L5, L6, L8 as mesh and scrambled, for NaN gradients on lines that run through unrelated patches.

No oracle and no tolerance is new.  The forward sweep goes by ``fuzz_parity.forward_matches`` against ``CO.power_map``; value +
gradient by ``test_gpu_grad._held_to_the_gradient_oracle`` (the rule of the lattice test) against ``CO.power_map_grad`` and by
``test_gpu_grad._same_flags_and_gradients`` between the culled and the exhaustive kernel; each sink product by the ``_same*`` of its own
test file against the folds of one ``many_walls_cases.gather``.  Beyond the oracles one identity is free: they are per cell, and the
kernels add a cell's candidates in candidate order whatever patch it sits in, so ``scrambled`` and ``flipped`` must give the mesh's
result re-indexed, bit for bit -- sigmoid included.  ``test_conditions_hold_on_the_oracle_alone_cpu`` asserts the floors of
``irregular_grids.conditions``, the products' guards and the oracles' own equivariance without a GPU.

Oracle time, measured on the CPU machine: ``power_map_grad`` with its two nudged runs 0.05 - 0.8 s per (grid, mode, role), 24 s for
all 96; ``gather`` 0.1 - 0.4 s per run; the CPU test takes 20 s over its 16 cases.  On the MI355X a launch is milliseconds: the 62 GPU tests take 7 s together, the slowest
(a value + gradient case: three modes, three kernels each) 0.3 s.

Mutants (scratch builds, not committed; this module run once against each).  A: the patch's box in ``fwd_patch`` and in the sink
kernel's ``wave_prologue`` taken from lanes 0, 7, 56 and 63 instead of all 64 -- 17 of the 62 GPU tests fail: the forward sweep and
value + gradient of scene R on ``scrambled``, ``polar``, ``track_row`` and ``track_col`` with an RX grid (``txg_patch`` keeps its own
reduction), value + gradient of the four scrambled lattice scenes, the cotangent test, and the sink products on ``scrambled`` and
``track_row`` in both runs.  B: ``region_box_kernel`` reduces a region's four corner cells only -- 32 fail: the same families in both
roles, the sink products on ``polar`` as well, and the content-check test, whose launches answer for the scrambled grid.  Under
either mutant all 145 tests of ``test_gpu_forward.py``, ``test_gpu_lists.py`` and ``test_gpu_hidden.py`` pass.  ``sheared``,
``collapsed`` and ``flipped`` catch neither: an affine map or a reversal leaves a patch's corner cells the extremes of its box; they
are here for overlapping, empty and descending boxes.

Measured on the MI355X with the product library: all 62 pass.  On every family and in both roles the hard and hard_sigmoid maps
are bit-equal to ``CO.power_map`` in all four launch shapes, three launches in a row, with lists (leaf regions and last-segment
masks built every time) and without, and the sigmoid maps within their rule; ``scrambled`` and ``flipped`` are bit-equal to the
mesh's maps re-indexed in all three modes.  Value + gradient: values bit-equal (sigmoid within 1e-6), NaN positions identical and
gradients within the lattice test's bar on all 16 grids, for both NaN scans and the exhaustive kernel; culled and exhaustive
gradients bit-equal; ``scrambled`` bit-equal to the mesh re-indexed, NaN for NaN.  All sink products are bit-equal to their folds
on the five families, and the position adjoint's planes follow the permutation.  The solver sweep follows it in both gradient
modes and cut into chunks.  No kernel or host code had to change."""

import functools
import os
import sys

import numpy as np
import pytest

import field_position_vjp_oracle as PO
import irregular_grids as G
import many_walls_cases as MW
import test_gpu_coherent_field as T_CF
import test_gpu_field_position_vjp as T_PV
import test_gpu_power_angle as T_PA
import test_gpu_power_profile as T_PP
import test_gpu_strongest_paths as T_SP
from coherent_field_oracle import AMP_SQRT, CoherentField
from coherent_field_oracle import fold as cf_fold
from power_angle_oracle import AT_RX, AT_TX, PowerAngleProfile
from power_angle_oracle import fold as pa_fold
from strongest_paths_oracle import top_k
from test_field_position_vjp_cpu import bars, inv_list
from test_gpu_grad import _held_to_the_gradient_oracle, _same_flags_and_gradients
from test_gpu_lists import SHAPES

gpu = pytest.mark.gpu

F = np.float32
REGIONS = {"region_size": 1, "region_size_top": 2, "hidden_min_tiles": 0}  # leaf regions of one patch: lists on grids this small
LAUNCH_SHAPES = dict(SHAPES, cut_in_parts={"split_max_tiles": 0, "sched_min_tiles": 1, "heavy_split": 8})
FORWARD = [(mode, 0, 2) for mode in G.MODES] + [(mode, 2, 3) for mode in ("hard", "hsig")]
REINDEXED = ("scrambled", "flipped")  # the families that are the mesh's cells in another order

# the sink sweep: scene R under the candidate mask and the coefficients of test_shared_geometry_serves_the_bits_of_the_loop_cpu
SINK_FAMILIES = ("scrambled", "sheared", "polar", "track_row", "collapsed")
SINK_RUNS = (("hard", "rx"), ("hsig", "tx"))
MASKED = (3, 8)
INV_20 = F(1) / F(0.05)
NF = 9  # a full chunk of 8 wavelengths plus one


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    """Bit for bit, NaN for NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _role_id(role):
    from differt2d_amd import _lib as L

    return L.GRID_TX if role == "tx" else L.GRID_RX


# ---- the sink sweep's oracle inputs and folds, each behind its guard -------------------------------------------------------------------
def _coef():
    coef = (0.2 + 0.05 * np.arange(14)).astype(F)
    coef[4] = -coef[4]
    return coef


@functools.lru_cache(maxsize=None)
def sink_inputs(family, mode, role):
    """One ``gather`` per run: what every product of the run is folded from."""
    fixed, walls = G.scene("R")
    return MW.gather(walls, fixed, *G.grid("R", family), 0, 2, role, MASKED, MW.MODES[mode], _coef())


def _shape(family):
    return G.grid("R", family)[0].shape


def sink_conditions(family, mode, role):
    inp = sink_inputs(family, mode, role)
    live = ~(inp.T == 0)
    contributing = int(live.any(axis=1).sum())
    lit = float(live.any(axis=0).mean())
    assert contributing >= 8 and live[1:1 + 12].any() and live[1 + 12:].any() and lit >= 0.7, (family, mode, role, contributing, lit)  # all three orders take part
    assert not any(o in MASKED for cand in inp.cands for o in cand) and len(inp.cands) == 1 + 12 + 12 * 11
    return dict(candidates=len(inp.cands), contributing=contributing, lit=round(lit, 2), records=int(live.sum()))


@functools.lru_cache(maxsize=None)
def want_strongest_paths(family, mode, role):
    sink_conditions(family, mode, role)
    inp = sink_inputs(family, mode, role)
    sp = top_k(inp.cands, inp.T, inp.Rl, inp.total, 3, _shape(family))
    assert (sp.count > 3).mean() > 1 / 4 and (sp.order[:3] == 2).any()  # k = 3 cuts real lists, and double reflections are kept
    return sp


@functools.lru_cache(maxsize=None)
def want_power_profile(family, mode, role):
    sink_conditions(family, mode, role)
    out = sink_inputs(family, mode, role).profile
    assert np.count_nonzero(out.reshape(MW.PROFILE[2], -1).any(axis=1)) >= 12  # (the small scenes' own guard: 12 of 24 bins occupied)
    return out


@functools.lru_cache(maxsize=None)
def want_coherent_field(family, mode, role):
    sink_conditions(family, mode, role)
    inp = sink_inputs(family, mode, role)
    cf = CoherentField(*(a.reshape(_shape(family)) for a in cf_fold(inp.T, inp.Rl, INV_20, AMP_SQRT)))
    assert np.count_nonzero(cf.im) > cf.im.size // 3 and np.count_nonzero(cf.re) > cf.re.size // 3
    return cf


@functools.lru_cache(maxsize=None)
def want_power_angle(family, mode, role):
    sink_conditions(family, mode, role)
    inp = sink_inputs(family, mode, role)
    out, total = pa_fold(inp.T, inp.D, AT_TX if role == "tx" else AT_RX, T_PA.ORIGIN_ODD, 12)
    pa = PowerAngleProfile(out.reshape((12,) + _shape(family)), total.reshape(_shape(family)))
    assert ((pa.bins != 0).sum(axis=0) >= 2).mean() > 1 / 4  # (random7's guard: a quarter of the cells have power in two or more bins)
    return pa


@functools.lru_cache(maxsize=None)
def position_bars(family):
    """The cotangent planes of the position adjoint; ``scrambled`` gets the mesh's, scrambled by the same permutation."""
    if family == "scrambled":
        rb, ib = position_bars("mesh")
        out = tuple(np.ascontiguousarray(np.stack([G.to_mesh_order(p, "R", "scrambled") for p in a])) for a in (rb, ib))
    else:
        out = bars(NF, _shape(family), 4000 + NF)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_field_position_vjp(family, mode, role):
    assert mode == "hard"
    sink_conditions(family, mode, role)
    inp = sink_inputs(family, mode, role)
    args = (inp.T, inp.Rl, inp.D, "received_power", MW.HEIGHT, inv_list(NF), *position_bars(family), AMP_SQRT, role)
    PO.guards(inp.T, inp.Rl, inp.D, role, PO.physics(*args), 2)
    return PO.restate(*args)


SINK_WANTS = (want_strongest_paths, want_power_profile, want_coherent_field, want_power_angle)


# ---- a. everything the GPU tests assume of the oracles, without a GPU -------------------------------------------------------------------
@pytest.mark.parametrize("scene,family", G.VG_GRIDS, ids=[f"{s}-{f}" for s, f in G.VG_GRIDS])
def test_conditions_hold_on_the_oracle_alone_cpu(scene, family):
    """The floors of ``irregular_grids.conditions`` for every (scene, grid, mode, role) the GPU tests use, the guards of the sink
    products, and the oracles' own equivariance: on ``scrambled`` they return the mesh's result re-indexed, bit for bit."""
    for mode in G.MODES:
        for role in G.ROLES:
            print(f"{scene} {family} {mode} {role}: {G.conditions(scene, family, mode, role)}")
            if family in REINDEXED:
                here, mesh = G.oracle_vg(scene, family, mode, role), G.oracle_vg(scene, "mesh", mode, role)
                for k in G.VG:
                    assert _same(here[k], G.to_mesh_order(mesh[k], scene, family)), (scene, family, mode, role, k)
    if scene != "R":
        return
    for mode, lo, hi in FORWARD:
        for role in G.ROLES:
            want = G.oracle_forward("R", family, mode, role, lo, hi)
            assert (want != 0).mean() >= 0.7, (family, mode, role, lo, hi)  # (orders 2..3 alone light the room too)
            if family in REINDEXED:
                assert _same(want, G.to_mesh_order(G.oracle_forward("R", "mesh", mode, role, lo, hi), "R", family))
    if family in SINK_FAMILIES:
        for mode, role in SINK_RUNS:
            inp = sink_inputs(family, mode, role)
            print(f"sink sweep {family} {mode} {role}: {sink_conditions(family, mode, role)}, oracle inputs in {inp.seconds:.1f} s")
            for want in SINK_WANTS:
                want(family, mode, role)
            if mode == "hard":
                want_field_position_vjp(family, mode, role)
    if family == "scrambled":
        p = G.permutation(G.grid("R", "mesh")[0].size)
        fixed, walls = G.scene("R")
        for mode, role in SINK_RUNS:
            here = sink_inputs("scrambled", mode, role)
            mesh = MW.gather(walls, fixed, *G.grid("R", "mesh"), 0, 2, role, MASKED, MW.MODES[mode], _coef())
            for k in ("T", "Rl", "total", "Tc", "totalc"):
                a, b = getattr(here, k), getattr(mesh, k)
                assert np.array_equal(_bits(a), _bits(b[..., p])), (mode, role, k)


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes():
    """One context per launch shape, each with leaf regions of one patch and the last-segment masks on grids this small, and one
    that enumerates every prefix in every patch."""
    from differt2d_amd.engine import Context

    ctxs = {}
    try:
        for name, opts in dict(LAUNCH_SHAPES, no_lists={"region_lists": 0}).items():
            c = ctxs[name] = Context(0)
            for k, v in dict({} if name == "no_lists" else REGIONS, **opts).items():
                c.set_option(k, v)
        yield ctxs
    finally:
        for c in ctxs.values():
            c.close()


@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


# ---- b. the forward sweep -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("role", G.ROLES)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_forward_sweep(shapes, family, role):
    """Every launch shape, three launches in a row (the third with work history, cut patches and last-segment masks), against the
    oracle; with and without lists; ``scrambled`` and ``flipped`` against the mesh re-indexed."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    from fuzz_parity import forward_matches

    fixed, walls = G.scene("R")
    X, Y = G.grid("R", family)
    Xm, Ym = G.grid("R", "mesh")
    for c in shapes.values():
        c.set_scene(walls)
    for mode, lo, hi in FORWARD:
        kw = dict(min_order=lo, max_order=hi, grid_role=_role_id(role), **G.MODES[mode])
        want = G.oracle_forward("R", family, mode, role, lo, hi)
        off = shapes["no_lists"].power_map(fixed, X, Y, **kw)
        assert shapes["no_lists"].debug_region_stats()["leaf_regions"] == 0
        assert forward_matches(off, want, kw), (family, role, mode, lo, hi, "no lists", int((off != want).sum()))
        for name in LAUNCH_SHAPES:
            c = shapes[name]
            tag = (family, role, mode, lo, hi, name)
            if family in REINDEXED:
                mesh = c.power_map(fixed, Xm, Ym, **kw)
            got = [c.power_map(fixed, X, Y, **kw) for _ in range(3)]
            st = c.debug_region_stats()
            assert st["leaf_regions"] > 0, (tag, st)  # lists were really built
            if role == "rx" and hi >= 2:
                assert c.hidden_masks()[1], tag  # ... and so were the last-segment masks
            assert forward_matches(got[0], want, kw), (tag, int((got[0] != want).sum()))
            assert _same(got[1], got[0]) and _same(got[2], got[0]), tag
            assert _same(got[0], off), (tag, "lists change bits", int((got[0] != off).sum()))
            if family in REINDEXED:
                assert _same(got[0], G.to_mesh_order(mesh, "R", family)), (tag, "differs from the mesh's result re-indexed")


# ---- c. value + gradient ------------------------------------------------------------------------------------------------------------------
def _vg_runs(ctx, scene, family, mode, role, cotangent=None):
    """``(culled with the two-level NaN scan, culled with one wave per patch, exhaustive)`` on one grid."""
    fixed, walls = G.scene(scene)
    X, Y = G.grid(scene, family)
    kw = dict(min_order=0, max_order=2, grid_role=_role_id(role), cotangent=cotangent, **G.MODES[mode])
    ctx.set_scene(walls)
    out = []
    try:
        for nan_scan, strict in ((1, False), (2, False), (1, True)):
            ctx.set_option("nan_scan", nan_scan)
            out.append(ctx.value_and_grads(fixed, X, Y, strict_nan=strict, **kw))
    finally:
        ctx.set_option("nan_scan", 1)
    return out


def _reindexed(res, scene, family):
    return dict(res, value=G.to_mesh_order(res["value"], scene, family), grad_rx=G.to_mesh_order(res["grad_rx"], scene, family))


@gpu
@pytest.mark.parametrize("role", G.ROLES)
@pytest.mark.parametrize("scene,family", G.VG_GRIDS, ids=[f"{s}-{f}" for s, f in G.VG_GRIDS])
def test_value_and_gradient(ctx, scene, family, role):
    """The culled kernel under both shapes of the NaN scan and the exhaustive kernel against ``CO.power_map_grad`` by the lattice
    test's rule, the culled against the exhaustive one, and ``scrambled`` / ``flipped`` against the mesh re-indexed."""
    for mode in G.MODES:
        G.conditions(scene, family, mode, role)
        o = G.oracle_vg(scene, family, mode, role)
        tag = (scene, family, mode, role)
        runs = _vg_runs(ctx, scene, family, mode, role)
        compared = [_held_to_the_gradient_oracle(r, o["value"], o["grad"], o["gabs"], o["kink"], o["stable"], G.MODES[mode]["function"], tag + (i,))
                    for i, r in enumerate(runs)]
        for i in (0, 1):
            _same_flags_and_gradients(runs[i], runs[2], f"{tag} culled (nan_scan {i + 1}) against exhaustive")
        if family in REINDEXED:
            mesh = _vg_runs(ctx, scene, "mesh", mode, role)
            for i, (here, there) in enumerate(zip(runs, mesh)):
                _same_flags_and_gradients(here, _reindexed(there, scene, family), f"{tag} run {i} against the mesh re-indexed")
        print(f"{scene} {family} {mode} {role}: {compared[0]} of {o['value'].size} gradients compared, {int(np.isnan(o['grad']).any(-1).sum())} NaN cells")


@gpu
def test_value_and_gradient_with_a_cotangent_that_follows_the_scramble(ctx):
    """A cotangent that differs cell by cell, scrambled by the grid's permutation: the same values and per-cell gradients re-indexed,
    the same scene VJP within the tolerance of sums in another order -- and not the VJP of a cotangent of ones."""
    shape = G.grid("R", "mesh")[0].shape
    cot = (np.random.default_rng(11).random(shape) + 0.5).astype(F)
    cot_s = np.ascontiguousarray(G.to_mesh_order(cot, "R", "scrambled"))
    for mode, role in (("hsig", "rx"), ("hard", "tx")):
        mesh = _vg_runs(ctx, "R", "mesh", mode, role, cot)
        here = _vg_runs(ctx, "R", "scrambled", mode, role, cot_s)
        ones = _vg_runs(ctx, "R", "scrambled", mode, role)
        for i, (a, b) in enumerate(zip(here, mesh)):
            _same_flags_and_gradients(a, _reindexed(b, "R", "scrambled"), f"cotangent {mode} {role} run {i}")
        fin = np.isfinite(here[2]["walls_bar"]) & np.isfinite(ones[2]["walls_bar"])
        assert fin.any() and not np.allclose(here[2]["walls_bar"][fin], ones[2]["walls_bar"][fin], rtol=1e-3, atol=0)


# ---- d. the sink sweep ----------------------------------------------------------------------------------------------------------------------
def _sink_setup(ctx, family, mode, role):
    from differt2d_amd.engine import make_params

    fixed, walls = G.scene("R")
    allowed = np.ones(len(walls), np.uint8)
    allowed[list(MASKED)] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    ctx.set_reflection_coefs(None)
    ctx.set_grid(*G.grid("R", family))
    return make_params(min_order=0, max_order=2, fun="received_power", grid_role=_role_id(role), **MW.MODES[mode], **MW.FUN_KW), fixed


def _total_is_the_fused_map(ctx, params, fixed, total):
    ctx.launch(params, fixed)
    fused = ctx.get_map()
    assert np.array_equal(_bits(total), _bits(fused)) and np.count_nonzero(fused) > fused.size // 3


@gpu
@pytest.mark.parametrize("mode,role", SINK_RUNS, ids=[f"{m}-{r}" for m, r in SINK_RUNS])
@pytest.mark.parametrize("family", SINK_FAMILIES)
def test_sink_products(ctx, family, mode, role):
    """``power_sink_kernel`` (``wave_prologue``'s box): every product by its own rule against the folds of one ``gather``; every
    ``total`` plane also against ``launch`` + ``get_map``; on ``scrambled`` the position adjoint's ``cell_bar`` against the mesh's."""
    inp = sink_inputs(family, mode, role)
    shape = _shape(family)
    try:
        params, fixed = _sink_setup(ctx, family, mode, role)
        # valid_paths: the records are the oracle's non-zero validities, cell by cell, with their wall sequences; lengths by bits
        sink_conditions(family, mode, role)
        rec = ctx.valid_paths(params, fixed)
        live = ~(inp.T == 0)
        want = {(int(cell),) + tuple(int(o) for o in inp.cands[ci]) for ci, cell in zip(*np.nonzero(live))}
        got = {(int(cell),) + tuple(int(o) for o in cand[:order]) for cell, cand, order in zip(rec["cell"], rec["cand"], rec["order"])}
        assert len(got) == len(rec["cell"]) == live.sum() and got == want
        rank = {tuple(int(o) for o in cand): ci for ci, cand in enumerate(inp.cands)}
        at = np.array([rank[tuple(int(o) for o in cand[:order])] for cand, order in zip(rec["cand"], rec["order"])])
        assert np.array_equal(_bits(rec["length"]), _bits(inp.Rl[at, rec["cell"]]))
        # strongest_paths, k = 3
        sp = ctx.strongest_paths(params, fixed, 3)
        T_SP._same(sp, want_strongest_paths(family, mode, role))
        _total_is_the_fused_map(ctx, params, fixed, sp.total)
        # power_profile
        T_PP._same_bits(ctx.power_profile(params, fixed, *MW.PROFILE), want_power_profile(family, mode, role))
        # coherent_field
        cf = ctx.coherent_field(params, fixed, INV_20, "sqrt")
        T_CF._same(cf, want_coherent_field(family, mode, role))
        _total_is_the_fused_map(ctx, params, fixed, cf.total)
        # power_angle, twelve bins from an origin that is no bin multiple, at the cells' end
        pa = ctx.power_angle(params, fixed, role, T_PA.ORIGIN_ODD, 12)
        T_PA._same(pa, want_power_angle(family, mode, role))
        _total_is_the_fused_map(ctx, params, fixed, pa.total)
        if mode == "hard":
            tag = f"field_position_vjp {family} {mode} {role}"
            pv = ctx.field_position_vjp(params, fixed, inv_list(NF), *position_bars(family), "sqrt")
            T_PV._same_planes(pv, want_field_position_vjp(family, mode, role), shape, tag)
            T_PV._fixed_bar_is_the_sum(pv, tag)
            if family == "scrambled":  # cell_bar is per cell: it follows the permutation
                ctx.set_grid(*G.grid("R", "mesh"))
                mesh = ctx.field_position_vjp(params, fixed, inv_list(NF), *position_bars("mesh"), "sqrt")
                for a, b in ((pv.cell_bar, mesh.cell_bar), (pv.fixed_terms, mesh.fixed_terms)):
                    assert np.array_equal(_bits(a), _bits(G.to_mesh_order(b, "R", "scrambled"))), tag
    finally:
        ctx.set_candidate_mask(None)
    print(f"sink sweep {family} {mode} {role}: {len(rec['cell'])} records, all products bit-equal")


# ---- e. the Python layer and the content check of the grid ---------------------------------------------------------------------------------
@gpu
def test_scene_methods_on_a_sheared_grid(ctx):
    from differt2d_amd import logic
    from differt2d_amd.geometry import Point
    from differt2d_amd.scene import Scene
    from differt2d_amd.utils import received_power

    fixed, walls = G.scene("R")
    X, Y = G.grid("R", "sheared")
    ctx.set_scene(walls)
    for mode in G.MODES:
        kw = G.MODES[mode]
        for role in G.ROLES:
            scene = Scene.from_walls_array(walls)
            sweep = (scene.with_transmitters(tx=Point(xy=fixed)).accumulate_on_receivers_grid_over_paths if role == "rx" else
                     scene.with_receivers(rx=Point(xy=fixed)).accumulate_on_transmitters_grid_over_paths)
            got = sweep(X, Y, fun=received_power, reduce_all=True, min_order=0, max_order=2, approx=kw["approx"], function=getattr(logic, kw["function"]))
            want = ctx.power_map(fixed, X, Y, min_order=0, max_order=2, grid_role=_role_id(role), **kw)
            assert np.asarray(got).dtype == F and np.array_equal(_bits(got), _bits(want)), (mode, role)
            assert (want != 0).mean() >= 0.7


@gpu
def test_a_scrambled_grid_of_the_same_shape_is_not_the_resident_grid(ctx):
    """``set_grid`` of ``scrambled`` after ``mesh``: the same shape, other bytes -- no reuse, and the next launch answers for the new
    grid; the same through the versioned route that immutable arrays take."""
    from differt2d_amd.engine import _immutable, make_params

    fixed, walls = G.scene("R")
    ctx.set_scene(walls)
    kw = dict(min_order=0, max_order=2, **G.MODES["hsig"])
    p = make_params(**kw)
    want = {f: G.oracle_forward("R", f, "hsig", "rx", 0, 2) for f in ("mesh", "scrambled")}
    writable = {f: tuple(a.copy() for a in G.grid("R", f)) for f in want}
    frozen = {f: G.grid("R", f) for f in want}
    assert all(_immutable(a) for f in want for a in frozen[f]) and not any(_immutable(a) for f in want for a in writable[f])

    def launch(grid, family):
        ctx.set_grid(*grid[family])
        ctx.launch(p, fixed)
        assert _same(ctx.get_map(), want[family]), family

    launch(writable, "mesh")
    n = ctx.grid_reuses()
    launch(writable, "scrambled")  # byte for byte against the resident copy: other bytes
    assert ctx.grid_reuses() == n
    launch(writable, "scrambled")
    assert ctx.grid_reuses() == n + 1  # (the counter does count: the same bytes again are a reuse)
    launch(writable, "mesh")
    assert ctx.grid_reuses() == n + 1
    launch(frozen, "scrambled")  # d2d_set_grid_versioned with a new token
    assert ctx.grid_reuses() == n + 1
    launch(frozen, "mesh")
    assert ctx.grid_reuses() == n + 1
    launch(frozen, "mesh")  # the same immutable arrays: recognised by identity
    assert ctx.grid_reuses() == n + 2


# ---- f. the solver sweeps: equivariance only ------------------------------------------------------------------------------------------------
@gpu
def test_solver_sweep_follows_a_scramble_of_its_grid():
    """MinPath, 20 steps, hard_sigmoid, orders 0..2 among three walls -- the first three sides of ``Scene.square_scene()``, the room
    of ``test_gpu_opt.py`` -- on a 19 x 13 mesh against its scramble: values and per-cell gradients re-indexed bit for bit in both
    ``opt_grad_mode``s, and with ``opt_traj_mb = 1``, which cuts the 247 cells into chunks of 192 and 55.  (With the RIS and its two
    vertices of ``test_gpu_opt._ris_scene`` the forward-tangent kernel returns NaN in every cell at order 2, on the mesh already,
    where the reverse kernel and the C oracle are finite: no ground for a comparison of gradients, so they stay out.)"""
    from differt2d_amd.engine import default_context
    from differt2d_amd.scene import Scene
    from test_gpu_opt import _scene_tables

    room = Scene.square_scene()
    scene = Scene(transmitters=room.transmitters, receivers={}, objects=list(room.objects)[:3])
    xys, kind, phi = _scene_tables(scene)
    X, Y = np.meshgrid(np.linspace(0.07, 0.93, 19).astype(F), np.linspace(0.11, 0.89, 13).astype(F))
    cands = scene.all_path_candidates(min_order=0, max_order=2)
    rng = np.random.default_rng(3)
    theta0 = [np.pad(rng.random(len(c), dtype=F), (0, 4 - len(c))) for c in cands]
    per_cell = 4 * 20 * sum(len(c) for c in cands)  # floats of trajectory per cell (Adam: 4 per step and unknown, one unknown per wall)
    assert len(cands) == 1 + 3 + 6 and max(64, (1 << 20) // (4 * per_cell) // 64 * 64) == 192 < X.size == 247
    p = np.random.default_rng(G.SCRAMBLE_SEED).permutation(X.size)
    Xs, Ys = (np.ascontiguousarray(a.reshape(-1)[p].reshape(a.shape)) for a in (X, Y))
    fixed = scene.transmitters["tx"].xy
    ctx = default_context()
    ctx.set_scene(xys, kind, phi)
    ctx.set_candidate_mask(None)
    ctx.set_theta0(theta0)
    kw = dict(solver="min", steps=20, min_order=0, max_order=2, approx=True)
    results = []
    try:
        for grad_mode, traj_mb in ((0, 16384), (1, 16384), (0, 1)):
            ctx.set_option("opt_grad_mode", grad_mode)
            ctx.set_option("opt_traj_mb", traj_mb)
            mesh = ctx.value_and_grads(fixed, X, Y, **kw)
            here = ctx.value_and_grads(fixed, Xs, Ys, **kw)
            assert _same(here["value"], mesh["value"].reshape(-1)[p].reshape(X.shape)), (grad_mode, traj_mb)
            assert _same(here["grad_rx"], mesh["grad_rx"].reshape(-1, 2)[p].reshape(X.shape + (2,))), (grad_mode, traj_mb)
            # (the C oracle of this sweep has every cell lit and every gradient finite)
            assert np.isfinite(mesh["grad_rx"]).all() and np.abs(mesh["grad_rx"]).max() > 0 and (mesh["value"] != 0).all(), (grad_mode, traj_mb)
            results.append(mesh)
    finally:
        ctx.set_option("opt_grad_mode", 0)
        ctx.set_option("opt_traj_mb", 16384)
    assert _same(results[2]["value"], results[0]["value"]) and _same(results[2]["grad_rx"], results[0]["grad_rx"])  # chunks change no bit
