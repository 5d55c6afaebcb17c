"""Every product of ``power_sink_kernel`` beyond 64 walls (include/d2d.h: the ``d2d_*_launch`` sinks; ``sweep_order_culled*`` with
``RECORD``, ``prep_sink_sweep``).  The products' own test files run on at most 7 walls: one chunk of the culling loop, no wall index
above 6, no flush of the queue between prefixes at order 2, no scene past the 256-wall bit masks.  Here each product runs on the five
cases of ``tests/many_walls_cases.py`` -- 70 walls (two chunks, 4 830 candidates at order 2), the same under a candidate mask, 130 walls
from ``min_order = 1`` (three chunks), 260 walls (five chunks, past the masks) and order 2 alone among 40 of 260 walls -- and is held to
its existing oracle by that oracle's own rule: bit for bit where the product's test file asserts bits (its ``_same``), within the
derived bound where it asserts a bound (its ``_within``).  No oracle is restated: ``contributions()`` and its siblings and the
products' folds are called as they are, once per case, mode and role, and shared (``many_walls_cases.inputs_of``).

Every ``want_*`` below first asserts on the ORACLE alone that the comparison cannot pass on empty ground
(``many_walls_cases.conditions`` and the product's own guards); ``test_conditions_hold_on_the_oracle_alone_cpu`` runs exactly those
assertions without a GPU.  Every product with a ``total`` plane is also held to ``Context.launch`` + ``get_map`` by bits, and every
product is launched a second time after another product ran on the context, for the same bits.

Oracle time, measured on the CPU machine (the geometry of all candidates side by side, then the oracles' loops; seconds per
case, mode and role): random70 4.8 - 6.5, random70_masked 2.0 - 2.9, random130 21.9, random260 0.4, random260_o2 2.0 -- 56 s for the
eleven runs, and 83 s for the CPU half of this module with the products' folds and guards (22 s) and the 5 s of
``test_shared_geometry_serves_the_bits_of_the_loop_cpu``.  The plain candidate-by-candidate loop takes 44 s for ONE run of random70
and minutes for random130, which is why the geometry is shared (``many_walls_cases`` says how).  The first test that touches a run
pays for its inputs (random130: 10 s beside the GPU, the one test above a few seconds); a GPU launch is milliseconds, and the 171 GPU
tests take 38 s together.

Measured on the MI355X: every plane-valued product is bit-equal to its oracle in all eleven runs; ``field_coefs_vjp`` is within
0.12 - 0.26 of its bound, ``material_eps_vjp`` within 0.30 - 0.38.  A build whose ``CoefGradSink`` and ``MaterialSink`` decode the
wall indices with ``0x3f`` in place of ``0xfff`` fails all 22 tests of those two products here and passes all 182 tests of
``test_gpu_material_response.py`` and ``test_gpu_field_coefs_vjp.py``.

``test_host_boundary_of_the_sink_sweep`` pins the largest scene the sink kernel takes: with the LDS limit the library derives from
the device (156 KB on the MI355X) ``tab_lds_bytes(N) = 16 (4 N + 1) + 512 <= lds_max`` gives N = 2487 accepted, 2488 refused, and
that is the pair the MI355X reports."""

import functools

import numpy as np
import pytest

import field_position_vjp_oracle as PO
import material_eps_vjp_oracle as EO
import material_response_oracle as MO
import test_gpu_array_frequency_response as T_AFR
import test_gpu_array_response as T_AR
import test_gpu_beam_response as T_BEAM
import test_gpu_coherent_field as T_CF
import test_gpu_field_coefs_vjp as T_CV
import test_gpu_field_position_vjp as T_PV
import test_gpu_frequency_response as T_FR
import test_gpu_material_eps_vjp as T_EV
import test_gpu_material_response as T_MR
import test_gpu_power_angle as T_PA
import test_gpu_power_profile as T_PP
import test_gpu_strongest_paths as T_SP
from array_frequency_response_oracle import ArrayFrequencyResponse
from array_frequency_response_oracle import fold_list as afr_fold_list
from array_frequency_response_oracle import guard as afr_guard
from array_response_oracle import ArrayResponse
from array_response_oracle import fold as ar_fold
from beam_response_oracle import BeamResponse
from beam_response_oracle import fold_list as beam_fold_list
from beam_response_oracle import guard as beam_guard
from coherent_field_oracle import AMP_LINEAR, AMP_SQRT, CoherentField
from coherent_field_oracle import fold as cf_fold
from field_coefs_vjp_oracle import coef_grad
from field_coefs_vjp_oracle import guards as cv_guards
from frequency_response_oracle import FrequencyResponse
from frequency_response_oracle import fold_list as fr_fold_list
from frequency_response_oracle import guard as fr_guard
from many_walls_cases import (CASES, FUN_KW, HEIGHT, MODES, PROFILE, RUN_IDS, RUNS, SPECIAL_WALLS, allowed_of, coefs_of, conditions, eps_of,
                              gather, inputs_of, permuted_upper, room_with_clutter, scene_of)
from power_angle_oracle import AT_RX, AT_TX, PowerAngleProfile
from power_angle_oracle import fold as pa_fold
from strongest_paths_oracle import top_k

gpu = pytest.mark.gpu

F = np.float32
AMPS = {"sqrt": AMP_SQRT, "linear": AMP_LINEAR}
INV_20 = F(1) / F(0.05)
NF = 9  # a full chunk of 8 wavelengths plus one
PER_OBJECT = "received_power_per_object"
HARD_RUNS = [r for r in RUNS if r[1] == "hard"]  # the position adjoint covers hard validity only
HARD_IDS = [i for i, r in zip(RUN_IDS, RUNS) if r[1] == "hard"]
ETX, ERX = T_BEAM.SHAPES["3x4"]  # 4 transmit and 3 receive elements: a 3 x 4 array
WTX, WRX = T_BEAM._book("2x3", "3x4")  # a 2 x 3 codebook: transmit beam 1 is all zero, receive beam 1 one-hot
by_runs = pytest.mark.parametrize("name,mode,role", RUNS, ids=RUN_IDS)


def _shape(name):
    return scene_of(name)[2].shape


def _amp(name):
    """The amplitude rule alternates over the cases, so that both appear at every wall count."""
    return "sqrt" if list(CASES).index(name) % 2 == 0 else "linear"


def _pol(name):
    return "te" if list(CASES).index(name) % 2 == 0 else "tm"


@functools.lru_cache(maxsize=None)
def _bars(name, nf):
    rng = np.random.default_rng(3000 + 31 * list(CASES).index(name) + nf)
    shape = (nf,) + _shape(name)
    rb, ib = rng.standard_normal(shape).astype(F), rng.standard_normal(shape).astype(F)
    rb.setflags(write=False)
    ib.setflags(write=False)
    return rb, ib


def _frozen(t):
    for a in t:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


def _upper_entries(name, lit, without=0):
    """The condition of the products with per-wall outputs, on the oracle's ``mag[..., N] > 0``: more than 10 entries of index >= 64
    carry terms -- at 70 walls a gradient of one entry per wall has six such entries, less ``without`` that the amplitude rule
    leaves without a term: then all of them do -- and at 260 walls one of index >= 256 does."""
    upper = np.asarray(lit)[..., 64:]
    assert upper.sum() >= min(11, upper.size - without), (name, np.argwhere(~upper))
    if CASES[name].n > 256:
        assert np.asarray(lit)[..., 256:].any(), name


# ---- the oracles, each behind its conditions ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def want_strongest_paths(name, mode, role, k, fun="received_power"):
    conditions(name, mode, role)
    inp = inputs_of(name, mode, role)
    T, total = (inp.T, inp.total) if fun == "received_power" else (inp.Tc, inp.totalc)
    sp = _frozen(top_k(inp.cands, T, inp.Rl, total, k, _shape(name)))
    assert (sp.cand[:3] >= 64).sum() >= 20  # the kept slots name upper walls
    if k == 8:
        assert (sp.count > 8).any() or CASES[name].hi < 2 or name == "random260_o2", sp.count.max()
    if fun == PER_OBJECT:
        assert (sp.power < 0).any() and not (sp.cand == SPECIAL_WALLS[name][1]).any()
    return sp


@functools.lru_cache(maxsize=None)
def want_coherent_field(name, mode, role):
    conditions(name, mode, role)
    inp = inputs_of(name, mode, role)
    cf = _frozen(CoherentField(*(a.reshape(_shape(name)) for a in cf_fold(inp.T, inp.Rl, INV_20, AMPS[_amp(name)]))))
    assert np.count_nonzero(cf.im) > cf.im.size // 3 and np.count_nonzero(cf.re) > cf.re.size // 3
    return cf


@functools.lru_cache(maxsize=None)
def want_coherent_field_per_object(name, mode, role):
    conditions(name, mode, role)
    inp = inputs_of(name, mode, role)
    cf = _frozen(CoherentField(*(a.reshape(_shape(name)) for a in cf_fold(inp.Tc, inp.Rl, INV_20, AMP_LINEAR))))
    assert (cf.total.reshape(-1).view(np.uint32) == inp.totalc.view(np.uint32)).all() and np.count_nonzero(cf.im) > cf.im.size // 3
    return cf


@functools.lru_cache(maxsize=None)
def want_frequency_response(name, mode, role):
    conditions(name, mode, role)
    inp = inputs_of(name, mode, role)
    re, im, total = fr_fold_list(inp.T, inp.Rl, T_FR.inv_list(NF), AMPS[_amp(name)])
    fr = _frozen(FrequencyResponse(re.reshape((-1,) + _shape(name)), im.reshape((-1,) + _shape(name)), total.reshape(_shape(name))))
    fr_guard(fr.re, fr.im)
    return fr


@functools.lru_cache(maxsize=None)
def want_power_profile(name, mode, role):
    conditions(name, mode, role)
    out = inputs_of(name, mode, role).profile
    assert np.count_nonzero(out.reshape(PROFILE[2], -1).any(axis=1)) >= 12  # (the small scenes' own guard: 12 of 24 bins occupied)
    return out


@functools.lru_cache(maxsize=None)
def want_power_angle(name, mode, role, end, origin, nbins):
    conditions(name, mode, role)
    inp = inputs_of(name, mode, role)
    out, total = pa_fold(inp.T, inp.D, AT_TX if end == "tx" else AT_RX, origin, nbins)
    pa = _frozen(PowerAngleProfile(out.reshape((nbins,) + _shape(name)), total.reshape(_shape(name))))
    assert ((pa.bins != 0).sum(axis=0) >= 2).mean() > 1 / 4  # (random7's guard: a quarter of the cells have power in two or more bins)
    return pa


@functools.lru_cache(maxsize=None)
def want_array_response(name, mode, role):
    conditions(name, mode, role)
    inp = inputs_of(name, mode, role)
    re, im, total = ar_fold(inp.T, inp.Rl, inp.D, INV_20, AMPS[_amp(name)], ETX, ERX)
    ar = _frozen(ArrayResponse(re.reshape(re.shape[:2] + _shape(name)), im.reshape(im.shape[:2] + _shape(name)), total.reshape(_shape(name))))
    assert np.count_nonzero(ar.im) > ar.im.size // 3 and np.count_nonzero(ar.re) > ar.re.size // 3
    return ar


@functools.lru_cache(maxsize=None)
def want_array_frequency_response(name, mode, role):
    conditions(name, mode, role)
    inp = inputs_of(name, mode, role)
    re, im, total = afr_fold_list(inp.T, inp.Rl, inp.D, T_BEAM._inv_list(NF), AMPS[_amp(name)], ETX, ERX)
    afr = _frozen(ArrayFrequencyResponse(re.reshape(re.shape[:3] + _shape(name)), im.reshape(im.shape[:3] + _shape(name)), total.reshape(_shape(name))))
    afr_guard(afr.re, afr.im)
    return afr


@functools.lru_cache(maxsize=None)
def want_beam_response(name, mode, role):
    conditions(name, mode, role)
    inp = inputs_of(name, mode, role)
    re, im, total = beam_fold_list(inp.T, inp.Rl, inp.D, T_BEAM._inv_list(NF), AMPS[_amp(name)], ETX, ERX, WTX, WRX)
    br = _frozen(BeamResponse(re.reshape(re.shape[:3] + _shape(name)), im.reshape(im.shape[:3] + _shape(name)), total.reshape(_shape(name))))
    assert not T_BEAM._bits(br.re[:, :, 1]).any() and not T_BEAM._bits(br.im[:, :, 1]).any()  # (transmit beam 1 is the all-zero one)
    beam_guard(br.re[:, :, [0, 2]], br.im[:, :, [0, 2]])
    return br


@functools.lru_cache(maxsize=None)
def want_material_response(name, mode, role):
    conditions(name, mode, role)
    inp = inputs_of(name, mode, role)
    walls = scene_of(name)[0]
    eps = eps_of(name, NF)
    args = (inp.cands, inp.T, inp.Rl, inp.S, MO.wall_normals(walls), T_MR.inv_list(NF))
    shape = _shape(name)
    planes = lambda re, im, total: MO.MaterialResponse(re.reshape((-1,) + shape), im.reshape((-1,) + shape), total.reshape(shape))  # noqa: E731
    mr = _frozen(planes(*MO.fold(*args, eps, T_MR.POLS[_pol(name)], AMPS[_amp(name)])))
    fr_guard(mr.re, mr.im)
    assert np.isfinite(mr.re).all() and np.isfinite(mr.im).all()
    # a lookup at a wrong upper index, or in a table of another row stride, changes bits
    moved = planes(*MO.fold(*args, permuted_upper(eps), T_MR.POLS[_pol(name)], AMPS[_amp(name)]))
    assert (moved.re.view(np.uint32) != mr.re.view(np.uint32)).sum() > mr.re.size // 10
    assert np.array_equal(moved.total.view(np.uint32), mr.total.view(np.uint32))
    return mr


@functools.lru_cache(maxsize=None)
def want_field_coefs_vjp(name, mode, role):
    conditions(name, mode, role)
    inp = inputs_of(name, mode, role)
    coef = coefs_of(name)
    amp = AMPS[_amp(name)]
    cg = coef_grad(inp.cands, inp.Sc, inp.Rl, coef, T_CV.inv_list(NF), *_bars(name, NF), amp)
    cv_guards(cg, np.ones_like(coef) if amp == AMP_LINEAR else coef, amp)
    _upper_entries(name, (cg.mag > 0) & (cg.coef_bar != 0), without=0 if amp == AMP_LINEAR else 1)  # (SQRT: no term through a zero coefficient)
    if amp == AMP_LINEAR:
        assert cg.mag[SPECIAL_WALLS[name][1]] > 0  # a zero coefficient HAS a gradient
    return cg


@functools.lru_cache(maxsize=None)
def want_material_eps_vjp(name, mode, role):
    conditions(name, mode, role)
    inp = inputs_of(name, mode, role)
    walls = scene_of(name)[0]
    eg = EO.eps_grad(inp.cands, inp.T, inp.Rl, inp.S, MO.wall_normals(walls), T_EV.inv_list(NF), eps_of(name, NF), *_bars(name, NF),
                     T_EV.POLS[_pol(name)], AMPS[_amp(name)])
    EO.guards(eg, inp.cands)
    _upper_entries(name, (eg.mag > 0) & (eg.eps_bar != 0))
    return eg


@functools.lru_cache(maxsize=None)
def want_field_position_vjp(name, mode, role):
    assert mode == "hard"
    conditions(name, mode, role)
    inp = inputs_of(name, mode, role)
    amp = AMPS[_amp(name)]
    args = (inp.T, inp.Rl, inp.D, "received_power", HEIGHT, T_PV.inv_list(NF), *_bars(name, NF), amp, role)
    PO.guards(inp.T, inp.Rl, inp.D, role, PO.physics(*args), CASES[name].hi)
    return PO.restate(*args)


WANTS = [want_coherent_field, want_coherent_field_per_object, want_frequency_response, want_power_profile, want_array_response,
         want_array_frequency_response, want_beam_response, want_material_response, want_field_coefs_vjp, want_material_eps_vjp]


# ---- the conditions, without a GPU ----------------------------------------------------------------------------------------------------
@by_runs
def test_conditions_hold_on_the_oracle_alone_cpu(name, mode, role):
    """Everything the GPU tests assert of the oracle before they look at a GPU result, for all five cases."""
    print(f"{name} {mode} {role}: {conditions(name, mode, role)}, oracle inputs in {inputs_of(name, mode, role).seconds:.1f} s")
    for want in WANTS:
        want(name, mode, role)
    for k in (3, 8):
        want_strongest_paths(name, mode, role, k)
    want_strongest_paths(name, mode, role, 3, PER_OBJECT)
    want_power_angle(name, mode, role, role, T_PA.ORIGIN_ODD, 12)
    if mode == "hard":
        want_field_position_vjp(name, mode, role)
    c = CASES[name]
    if c.masked:  # the masked walls still occlude: without them the line of sight reaches other cells
        from strongest_paths_oracle import contributions

        walls, fixed, X, Y = scene_of(name)
        kw = dict(min_order=0, max_order=0, grid_role=role, fun_kwargs=FUN_KW, **MODES[mode])
        with_them = contributions(walls, fixed, X, Y, **kw)[3]
        without = contributions(np.delete(walls, list(c.masked), axis=0), fixed, X, Y, **kw)[3]
        assert (with_them != without).any()


@pytest.mark.parametrize("mode,role", [("hard", "rx"), ("hsig", "tx")])
def test_shared_geometry_serves_the_bits_of_the_loop_cpu(mode, role):
    """A room of 5 pieces with 9 shortened walls, two of them masked, orders 0-2: what ``gather`` returns over the shared geometry
    against the same oracles run as they are, candidate by candidate."""
    from field_coefs_vjp_oracle import scale_contributions
    from object_coefs_oracle import coef_map
    from power_angle_oracle import directed_contributions
    from power_profile_oracle import profile_map
    from strongest_paths_oracle import contributions

    fixed, walls = room_with_clutter(14, 9, 0.3, (1, 4, 8, 12, 13))
    X, Y = scene_of("random260_o2")[2:]
    coef = (0.2 + 0.05 * np.arange(14)).astype(F)
    coef[4] = -coef[4]
    masked = (3, 8)
    got = gather(walls, fixed, X, Y, 0, 2, role, masked, MODES[mode], coef)
    kw = dict(min_order=0, max_order=2, grid_role=role, filter_nodes=set(masked), **MODES[mode])
    cands, T, Rl, total = contributions(walls, fixed, X, Y, fun="received_power", fun_kwargs=FUN_KW, **kw)
    D = directed_contributions(walls, fixed, X, Y, fun="received_power", fun_kwargs=FUN_KW, **kw)[2]
    S = MO.segment_contributions(walls, fixed, X, Y, fun="received_power", fun_kwargs=FUN_KW, **kw)[3]
    Sc = scale_contributions(walls, fixed, X, Y, HEIGHT, **kw)[1]
    Tc, totalc = contributions(walls, fixed, X, Y, fun=PER_OBJECT, coef=coef, fun_kwargs=dict(height=HEIGHT), **kw)[1::2]
    profile = profile_map(walls, fixed, X, Y, *PROFILE, fun="received_power", fun_kwargs=FUN_KW, **kw)
    cmap = np.ascontiguousarray(coef_map(walls, coef, fixed, X, Y, height=HEIGHT, **kw), F).reshape(-1)
    assert len(cands) == len(got.cands) == 1 + 12 + 12 * 11 and all(np.array_equal(a, b) for a, b in zip(cands, got.cands))
    for label, a, b in (("T", got.T, T), ("Rl", got.Rl, Rl), ("total", got.total, total), ("D", got.D, D), ("S", got.S, S), ("Sc", got.Sc, Sc),
                        ("Tc", got.Tc, Tc), ("totalc", got.totalc, totalc), ("profile", got.profile, profile), ("coef_map", got.totalc, cmap)):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), label
    live = ~(T == 0)
    assert live.any(axis=1).sum() > 20 and live[1 + 12:].any() and (Tc < 0).any()  # (double reflections and clutter take part)


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


def _setup(ctx, name, mode, role, fun="received_power"):
    """The case's scene, mask, coefficients and grid on the context; returns ``(params, fixed)``."""
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = scene_of(name)
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed_of(name))
    ctx.set_reflection_coefs(coefs_of(name) if fun == PER_OBJECT else None)
    ctx.set_grid(X, Y)
    c = CASES[name]
    extra = dict(height=HEIGHT) if fun == PER_OBJECT else FUN_KW
    return make_params(min_order=c.lo, max_order=c.hi, fun=fun, grid_role=T_SP._role_id(role), **MODES[mode], **extra), fixed


def _total_is_the_fused_map(ctx, params, fixed, total):
    ctx.launch(params, fixed)
    fused = ctx.get_map()
    assert np.array_equal(np.ascontiguousarray(total).view(np.uint32), fused.view(np.uint32)) and np.count_nonzero(fused) > fused.size // 3


def _another_product(ctx, params, fixed, profile=True):
    """A launch of another sink on the same context, between two launches of the product under test."""
    if profile:
        ctx.power_profile(params, fixed, 0.0, 4.0, 5)
    else:
        ctx.coherent_field(params, fixed, F(7.5), "linear")


@gpu
@pytest.mark.parametrize("k", [3, 8])
@by_runs
def test_strongest_paths(ctx, name, mode, role, k):
    want = want_strongest_paths(name, mode, role, k)
    params, fixed = _setup(ctx, name, mode, role)
    got = ctx.strongest_paths(params, fixed, k)
    T_SP._same(got, want)
    _total_is_the_fused_map(ctx, params, fixed, got.total)
    _another_product(ctx, params, fixed)
    T_SP._same(ctx.strongest_paths(params, fixed, k), got)
    print(f"strongest_paths {name} {mode} {role} k={k}: bit-equal; count max {want.count.max()}, {(want.cand >= 64).sum()} slots name walls >= 64")


@gpu
@by_runs
def test_strongest_paths_with_per_object_coefficients(ctx, name, mode, role):
    """TopSink with the D2D_FUN_RECEIVED_POWER_PER_OBJECT lookup: a negative and a zero coefficient on walls >= 64."""
    want = want_strongest_paths(name, mode, role, 3, PER_OBJECT)
    params, fixed = _setup(ctx, name, mode, role, PER_OBJECT)
    got = ctx.strongest_paths(params, fixed, 3)
    T_SP._same(got, want)
    _total_is_the_fused_map(ctx, params, fixed, got.total)


@gpu
@by_runs
def test_valid_paths(ctx, name, mode, role):
    """RecSink: the records are the oracle's non-zero validities, cell by cell, with their wall sequences."""
    conditions(name, mode, role)
    inp = inputs_of(name, mode, role)
    params, fixed = _setup(ctx, name, mode, role)
    rec = ctx.valid_paths(params, fixed)
    # received_power is valid * f with f > 0 and finite here: a contribution is non-zero exactly where the validity is
    live = ~(inp.T == 0)
    want = {(int(cell),) + tuple(int(o) for o in inp.cands[ci]) for ci, cell in zip(*np.nonzero(live))}
    got = {(int(cell),) + tuple(int(o) for o in cand[:order]) for cell, cand, order in zip(rec["cell"], rec["cand"], rec["order"])}
    assert len(got) == len(rec["cell"]) == live.sum() and got == want
    rank = {tuple(int(o) for o in cand): ci for ci, cand in enumerate(inp.cands)}
    at = np.array([rank[tuple(int(o) for o in cand[:order])] for cand, order in zip(rec["cand"], rec["order"])])
    assert np.array_equal(rec["length"].view(np.uint32), inp.Rl[at, rec["cell"]].view(np.uint32))


@gpu
@by_runs
def test_coherent_field(ctx, name, mode, role):
    want = want_coherent_field(name, mode, role)
    params, fixed = _setup(ctx, name, mode, role)
    got = ctx.coherent_field(params, fixed, INV_20, _amp(name))
    T_CF._same(got, want)
    _total_is_the_fused_map(ctx, params, fixed, got.total)
    _another_product(ctx, params, fixed)
    T_CF._same(ctx.coherent_field(params, fixed, INV_20, _amp(name)), got)
    print(f"coherent_field {name} {mode} {role} {_amp(name)}: bit-equal")


@gpu
@by_runs
def test_coherent_field_with_per_object_coefficients(ctx, name, mode, role):
    """FieldSink with the per-object lookup; its total is ``object_coefs_oracle.coef_map``, which the fused map equals too."""
    want = want_coherent_field_per_object(name, mode, role)
    params, fixed = _setup(ctx, name, mode, role, PER_OBJECT)
    got = ctx.coherent_field(params, fixed, INV_20, "linear")
    T_CF._same(got, want)
    _total_is_the_fused_map(ctx, params, fixed, got.total)
    print(f"coherent_field per object {name} {mode} {role}: bit-equal, and so is the fused map against coef_map")


@gpu
@by_runs
def test_frequency_response(ctx, name, mode, role):
    want = want_frequency_response(name, mode, role)
    params, fixed = _setup(ctx, name, mode, role)
    got = ctx.frequency_response(params, fixed, T_FR.inv_list(NF), _amp(name))
    T_FR._same(got, want)
    _total_is_the_fused_map(ctx, params, fixed, got.total)
    _another_product(ctx, params, fixed)
    T_FR._same(ctx.frequency_response(params, fixed, T_FR.inv_list(NF), _amp(name)), got)
    print(f"frequency_response {name} {mode} {role} {_amp(name)} nf={NF}: bit-equal")


@gpu
@by_runs
def test_power_profile(ctx, name, mode, role):
    want = want_power_profile(name, mode, role)
    params, fixed = _setup(ctx, name, mode, role)
    got = ctx.power_profile(params, fixed, *PROFILE)
    T_PP._same_bits(got, want)
    _another_product(ctx, params, fixed, profile=False)
    T_PP._same_bits(ctx.power_profile(params, fixed, *PROFILE), got)
    print(f"power_profile {name} {mode} {role}: bit-equal")


@gpu
@by_runs
def test_power_angle(ctx, name, mode, role):
    """Departure and arrival, twelve bins from an origin that is no bin multiple and eight from 0."""
    params, fixed = _setup(ctx, name, mode, role)
    for end, origin, nbins in (("tx", T_PA.ORIGIN_ODD, 12), ("rx", T_PA.ORIGIN_ODD, 12), (role, 0.0, 8)):
        want = want_power_angle(name, mode, role, end, origin, nbins)
        got = ctx.power_angle(params, fixed, end, origin, nbins)
        T_PA._same(got, want)
    _total_is_the_fused_map(ctx, params, fixed, got.total)
    _another_product(ctx, params, fixed)
    T_PA._same(ctx.power_angle(params, fixed, end, origin, nbins), got)
    print(f"power_angle {name} {mode} {role}: bit-equal")


@gpu
@by_runs
def test_array_response(ctx, name, mode, role):
    want = want_array_response(name, mode, role)
    params, fixed = _setup(ctx, name, mode, role)
    got = ctx.array_response(params, fixed, INV_20, ETX, ERX, _amp(name))
    T_AR._same(got, want)
    _total_is_the_fused_map(ctx, params, fixed, got.total)
    _another_product(ctx, params, fixed)
    T_AR._same(ctx.array_response(params, fixed, INV_20, ETX, ERX, _amp(name)), got)
    print(f"array_response {name} {mode} {role} {_amp(name)} 3x4: bit-equal")


@gpu
@by_runs
def test_array_frequency_response(ctx, name, mode, role):
    want = want_array_frequency_response(name, mode, role)
    params, fixed = _setup(ctx, name, mode, role)
    inv = T_BEAM._inv_list(NF)
    got = ctx.array_frequency_response(params, fixed, inv, ETX, ERX, _amp(name))
    T_AFR._same(got, want)
    _total_is_the_fused_map(ctx, params, fixed, got.total)
    _another_product(ctx, params, fixed)
    T_AFR._same(ctx.array_frequency_response(params, fixed, inv, ETX, ERX, _amp(name)), got)
    print(f"array_frequency_response {name} {mode} {role} {_amp(name)} 3x4 nf={NF}: bit-equal")


@gpu
@by_runs
def test_beam_response(ctx, name, mode, role):
    want = want_beam_response(name, mode, role)
    params, fixed = _setup(ctx, name, mode, role)
    inv = T_BEAM._inv_list(NF)
    got = ctx.beam_response(params, fixed, inv, ETX, ERX, WTX, WRX, _amp(name))
    T_BEAM._same(got, want)
    _total_is_the_fused_map(ctx, params, fixed, got.total)
    _another_product(ctx, params, fixed)
    T_BEAM._same(ctx.beam_response(params, fixed, inv, ETX, ERX, WTX, WRX, _amp(name)), got)
    print(f"beam_response {name} {mode} {role} {_amp(name)} 3x4, 2x3 beams, nf={NF}: bit-equal")


@gpu
@by_runs
def test_material_response(ctx, name, mode, role):
    want = want_material_response(name, mode, role)
    params, fixed = _setup(ctx, name, mode, role)
    inv, eps = T_MR.inv_list(NF), eps_of(name, NF)
    got = ctx.material_response(params, fixed, inv, eps, _pol(name), _amp(name))
    T_MR._same(got, want)
    _total_is_the_fused_map(ctx, params, fixed, got.total)
    _another_product(ctx, params, fixed)
    T_MR._same(ctx.material_response(params, fixed, inv, eps, _pol(name), _amp(name)), got)
    print(f"material_response {name} {mode} {role} {_pol(name)} {_amp(name)} nf={NF}: bit-equal")


@gpu
@by_runs
def test_field_coefs_vjp(ctx, name, mode, role):
    cg = want_field_coefs_vjp(name, mode, role)
    params, fixed = _setup(ctx, name, mode, role, PER_OBJECT)
    inv = T_CV.inv_list(NF)
    got = ctx.field_coefs_vjp(params, fixed, inv, *_bars(name, NF), _amp(name))
    T_CV._within(got, cg, f"field_coefs_vjp {name} {mode} {role} {_amp(name)} nf={NF}")
    _another_product(ctx, params, fixed)
    assert np.array_equal(T_CV._bits(ctx.field_coefs_vjp(params, fixed, inv, *_bars(name, NF), _amp(name))), T_CV._bits(got))


@gpu
@by_runs
def test_material_eps_vjp(ctx, name, mode, role):
    eg = want_material_eps_vjp(name, mode, role)
    params, fixed = _setup(ctx, name, mode, role)
    inv, eps = T_EV.inv_list(NF), eps_of(name, NF)
    got = ctx.material_eps_vjp(params, fixed, inv, eps, *_bars(name, NF), _pol(name), _amp(name))
    T_EV._within(got, eg, f"material_eps_vjp {name} {mode} {role} {_pol(name)} {_amp(name)} nf={NF}")
    _another_product(ctx, params, fixed)
    assert np.array_equal(T_EV._bits(ctx.material_eps_vjp(params, fixed, inv, eps, *_bars(name, NF), _pol(name), _amp(name))), T_EV._bits(got))


@gpu
@pytest.mark.parametrize("name,mode,role", HARD_RUNS, ids=HARD_IDS)
def test_field_position_vjp(ctx, name, mode, role):
    want = want_field_position_vjp(name, mode, role)
    params, fixed = _setup(ctx, name, mode, role)
    inv = T_PV.inv_list(NF)
    tag = f"field_position_vjp {name} {mode} {role} {_amp(name)} nf={NF}"
    got = ctx.field_position_vjp(params, fixed, inv, *_bars(name, NF), _amp(name))
    T_PV._same_planes(got, want, _shape(name), tag)
    T_PV._fixed_bar_is_the_sum(got, tag)
    _another_product(ctx, params, fixed)
    again = ctx.field_position_vjp(params, fixed, inv, *_bars(name, NF), _amp(name))
    assert all(np.array_equal(T_PV._bits(a), T_PV._bits(b)) for a, b in zip(again, got))
    print(f"{tag}: bit-equal")


# ---- the host's limits ------------------------------------------------------------------------------------------------------------------
BOUNDARY_FIXED = np.array([0.25, 0.5], F)


def _boundary_grid():
    return np.array([[0.75]], F), np.array([[0.5]], F)


def _boundary_walls(n, blocked=False):
    """``n`` short walls above y = 0.6, clear of the line of sight from (0.25, 0.5) to the one cell (0.75, 0.5) -- but the LAST wall,
    which crosses it if ``blocked``: the wall with the largest index decides the only candidate."""
    walls = room_with_clutter(n, 21, 0.02, ())[1]
    walls[:, :, 1] = F(0.6) + F(0.4) * walls[:, :, 1]
    walls[n - 1] = np.array([[0.5, 0.4], [0.5, 0.6]], F) + (F(0.0) if blocked else F(0.3))
    return walls


def _accepts(ctx, n, params):
    """Whether ``d2d_valid_paths`` takes a scene of ``n`` walls (the refusal comes before anything is launched)."""
    from differt2d_amd import _lib as L

    ctx.set_scene(_boundary_walls(n))
    try:
        ctx.valid_paths(params, BOUNDARY_FIXED)
    except L.D2DUnsupported as e:
        assert e.status == -4 and "d2d_valid_paths" in str(e) and "LDS" in str(e), str(e)
        return False
    return True


@gpu
def test_host_boundary_of_the_sink_sweep(ctx):
    """The largest scene ``prep_sink_sweep`` takes, searched from the refusal (the library has no getter for its LDS limit), through an
    EARLY product (``d2d_valid_paths``) and a LATE one that outlives ``d2d_set_scene`` (``d2d_power_angle_launch``).  A 1 x 1 grid at
    order 0: one candidate, whose validity the wall with the LARGEST index decides -- both ways."""
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params
    from power_angle_oracle import directed_contributions
    from strongest_paths_oracle import contributions

    params = make_params(min_order=0, max_order=0, **FUN_KW)
    fixed = BOUNDARY_FIXED
    X, Y = _boundary_grid()
    ctx.set_scene(_boundary_walls(64))
    ctx.set_candidate_mask(None)
    ctx.set_reflection_coefs(None)
    ctx.set_grid(X, Y)
    lo, hi = 64, 4095  # accepted, refused (4 095 walls take 262 KB of tables: more LDS than a CU has)
    assert _accepts(ctx, lo, params) and not _accepts(ctx, hi, params)
    for guess in (2487, 2488):  # the pair that 156 KB give: two probes in place of twelve
        if lo < guess < hi:
            lo, hi = (guess, hi) if _accepts(ctx, guess, params) else (lo, guess)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _accepts(ctx, mid, params) else (lo, mid)
    print(f"prep_sink_sweep: {lo} walls accepted, {hi} refused")
    lds = lambda n: 16 * (4 * n + 1) + 512  # noqa: E731 -- d2d_host::tab_lds_bytes
    assert lds(lo) <= 156 * 1024 < lds(hi) or hi < 2488, (lo, hi)  # (a device that grants less LDS has a pair of its own)
    for blocked in (True, False):
        walls = _boundary_walls(lo, blocked)
        cands, T, Rl, total = contributions(walls, fixed, X, Y, min_order=0, max_order=0, fun_kwargs=FUN_KW)
        D = directed_contributions(walls, fixed, X, Y, min_order=0, max_order=0, fun_kwargs=FUN_KW)[2]
        assert len(cands) == 1 and (total[0] == 0) == blocked
        ctx.set_scene(walls)
        rec = ctx.valid_paths(params, fixed)
        assert len(rec["cell"]) == (0 if blocked else 1)
        pa = ctx.power_angle(params, fixed, "tx", 0.0, 8)
        out, tot = pa_fold(T, D, AT_TX, 0.0, 8)
        T_PA._same(pa, PowerAngleProfile(out.reshape(8, 1, 1), tot.reshape(1, 1)))
        assert bool(pa.bins[0, 0, 0] != 0) != blocked  # (the cell lies due east of the transmitter: bin 0)
    assert rec["order"][0] == 0 and np.array_equal(rec["length"].view(np.uint32), Rl[0].view(np.uint32))
    # one wall more: refused, by name; the EARLY product's previous result is gone, the LATE one's still readable
    ctx.set_scene(_boundary_walls(hi))
    n = len(rec["cell"])
    again = {"cell": np.empty(n, np.int32), "valid": np.empty(n, F), "length": np.empty(n, F)}
    read = lambda: ctx._lib.d2d_get_valid_paths(ctx._ctx, n, again["cell"].ctypes.data, None, None, None, None,  # noqa: E731
                                                again["valid"].ctypes.data, again["length"].ctypes.data)
    assert read() == 0 and np.array_equal(again["length"].view(np.uint32), rec["length"].view(np.uint32))
    with pytest.raises(L.D2DUnsupported, match="d2d_valid_paths") as e:
        ctx.valid_paths(params, fixed)
    assert e.value.status == -4 and f"{hi} objects" in str(e.value)
    assert read() != 0
    with pytest.raises(L.D2DUnsupported, match="d2d_power_angle_launch") as e:
        ctx.power_angle(params, fixed, "tx", 0.0, 8)
    assert e.value.status == -4 and f"{hi} objects" in str(e.value)
    T_PA._same(ctx.get_power_angle(), pa)
