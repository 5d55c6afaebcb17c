"""The scenes of ``tests/test_gpu_sinks_many_walls.py`` and the oracle inputs that all its products share.

Scenes.  ``conftest.random_scene(n, seed)`` draws both ends of every wall in the unit square, so a wall is 0.52 long on average and
70 of them leave every cell of a grid dark (seed 1, hard validity: not one of the 4 901 candidates of orders 0-2 contributes
anywhere; at 260 walls, seeds 1-8, at most 7 of 261 do).  Shortening every wall alike lets the line of sight through but leaves
hardly a reflection (70 walls at a fifth of their length, seeds 1-4: at most 6 contributing candidates name a wall >= 64; order 2
alone among 40 of 260 walls: none or one contributes).  No seed meets the module's conditions on such scenes, which want twenty
contributing candidates through walls >= 64 and a third of the cells lit.  So a scene here is a room with clutter: the walls of
``random_scene(n, seed)``, each shortened about its midpoint to ``short`` of its length, except the walls at the case's ``room``
indices, which are the sides of the square [-0.05, 1.05]^2 cut into equal pieces, counter-clockwise, in index order.  The room's
pieces reflect into every cell, singly and doubly, at whatever wall indices the case puts them; the clutter fills the other indices
and occludes some of the paths.

Oracle time.  ``contributions()`` and its siblings call ``R.accumulate_candidate`` once per candidate, 9 ms at 70 walls and 17 ms at
130 (the occlusion test is a Python loop over the walls): 44 s for case A in one role and mode, minutes for case C.  The geometry of a
candidate -- ``valid``, the path's points, the loss -- does not depend on the path function, so ``shared_geometry`` computes it once
per case for all candidates of an order side by side, with ``oracle/ref.py``'s own batched pieces (``image_path`` on stacked walls and
``intersects_with_objects_batched``, composed as ``R.facc_batched`` composes them, which ``tests/test_oracle_batched.py`` pins to the
loop), and serves ``R.accumulate_candidate`` from that table while the unchanged oracles run: ``contributions``,
``directed_contributions``, ``segment_contributions`` and ``scale_contributions`` are all called as they are.
``test_shared_geometry_serves_the_bits_of_the_loop_cpu`` holds what is served to the plain loop bit for bit."""

import contextlib
import functools
import time
from collections import namedtuple

import numpy as np

from conftest import random_scene, unit_grid
from oracle import ref as R

F = np.float32
MODES = {"hard": dict(approx=False), "hsig": dict(approx=True, function="hard_sigmoid")}
HEIGHT = 0.25
FUN_KW = dict(r_coef=0.5, height=HEIGHT)  # received_power's keywords in every product of the module
BATCH = 2048  # candidates side by side: bounds the tables at a few tens of MB

Case = namedtuple("Case", "n seed short room grid lo hi masked runs")


def _every(n, mod, residues):
    return tuple(w for w in range(n) if w % mod in residues)


# room: the wall indices that hold the room's pieces; every other wall is random_scene's at ``short`` of its length.  masked: the
# walls the candidate mask takes out (they still occlude).  runs: the (mode, role) pairs the case is run in.
ALL4 = (("hard", "rx"), ("hard", "tx"), ("hsig", "rx"), ("hsig", "tx"))
ROOM70 = (6, 11, 22, 34, 38, 53, 64, 65, 66, 67, 68, 69)
CASES = {
    # 70 walls: a second chunk of 6 live lanes; 4 830 candidates at order 2, so the queue of 64 flushes between prefixes
    "random70": Case(70, 4, 0.1, ROOM70, (11, 9), 0, 2, (), ALL4),
    # 21 of the 70 out, all below 64, the room's pieces 11 and 34 among them: Nc = 49, cw[p] != p from p = 0 on
    "random70_masked": Case(70, 4, 0.1, ROOM70, (11, 9), 0, 2, (0, 2) + _every(64, 10, (1, 4, 7)), ALL4),
    # 130 walls, min_order = 1: three chunks, the last of 2 lanes
    "random130": Case(130, 5, 0.06, (3, 40, 66, 70, 75, 88, 99, 101, 110, 120, 128, 129), (9, 9), 1, 2, (), (("hsig", "tx"),)),
    # 260 walls: past the 256-wall bit masks; five chunks, the last of 4 lanes
    "random260": Case(260, 11, 0.03, _every(260, 9, (4,)), (9, 9), 0, 1, (), (("hard", "rx"),)),
    # 260 walls of which the 40 of the room are candidates, 8 per chunk (w mod 13 in {2, 9}; 256 is one of them): order 2 alone
    "random260_o2": Case(260, 7, 0.03, _every(260, 13, (2, 9)), (9, 5), 2, 2, tuple(w for w in range(260) if w % 13 not in (2, 9)),
                         (("hsig", "rx"),)),
}
RUNS = [(name, mode, role) for name, c in CASES.items() for mode, role in c.runs]
RUN_IDS = [f"{name}-{mode}-{role}" for name, mode, role in RUNS]


def room_pieces(count, lo=-0.05, hi=1.05):
    """``[count, 2, 2]``: the sides of the square ``[lo, hi]^2`` cut into equal pieces (the first ``count % 4`` sides into one piece
    more), counter-clockwise from the lower left corner."""
    corners = np.array([[lo, lo], [hi, lo], [hi, hi], [lo, hi], [lo, lo]], np.float64)
    out = []
    for side in range(4):
        m = count // 4 + (1 if side < count % 4 else 0)
        t = np.linspace(0.0, 1.0, m + 1)[:, None]
        p = corners[side] + t * (corners[side + 1] - corners[side])
        out += [np.stack([p[i], p[i + 1]]) for i in range(m)]
    return np.array(out).astype(F)


def room_with_clutter(n, seed, short, room):
    """``(fixed, walls)``: ``random_scene(n, seed)`` with every wall shortened about its midpoint to ``short`` of its length and the
    walls at the indices ``room`` replaced by the room's pieces."""
    fixed, walls = random_scene(n, seed=seed)
    mid = (walls[:, :1] + walls[:, 1:]) * F(0.5)
    walls = (mid + (walls - mid) * F(short)).astype(F)
    if room:
        walls[list(room)] = room_pieces(len(room))
    return fixed, walls


@functools.lru_cache(maxsize=None)
def scene_of(name):
    """``(walls, fixed end point, X, Y)``, read-only."""
    c = CASES[name]
    fixed, walls = room_with_clutter(c.n, c.seed, c.short, c.room)
    X, Y = unit_grid(*c.grid)  # 11 x 9, 9 x 9, 9 x 5: partial 8 x 8 patches on both sides
    for a in (walls, fixed, X, Y):
        a.setflags(write=False)
    return walls, fixed, X, Y


def allowed_of(name):
    """The candidate mask of a case (uint8 per wall), or ``None``."""
    c = CASES[name]
    if not c.masked:
        return None
    allowed = np.ones(c.n, np.uint8)
    allowed[list(c.masked)] = 0
    return allowed


def coefs_of(name):
    """Reflection coefficients that differ wall by wall (0.2 .. 0.9), with a negative one and a zero at indices >= 64 (and, at 260
    walls, a negative one at an index >= 256) on walls that carry contributions -- ``conditions`` asserts that they do."""
    n = CASES[name].n
    coef = (0.2 + 0.7 * ((np.arange(n) * 37) % 101) / 101.0).astype(F)
    neg, zero = SPECIAL_WALLS[name][:2]
    coef[neg], coef[zero] = F(-0.7), F(0.0)
    for w in SPECIAL_WALLS[name][2:]:
        coef[w] = -coef[w]
    return coef


# (negative, zero[, more negatives]) per case: walls >= 64 that carry contributions in every run of the case
SPECIAL_WALLS = {"random70": (65, 64), "random70_masked": (65, 64), "random130": (88, 101), "random260": (76, 112, 256),
                 "random260_o2": (132, 106, 256)}


def eps_of(name, nf):
    """Permittivities that differ wall by wall and row by row: ``eps[f, w] = 2 + w / 16 + 0.11 f - j (0.1 + w / 512 + 0.02 f)``,
    complex64 ``[nf, n]``."""
    f, w = np.arange(nf)[:, None], np.arange(CASES[name].n)[None, :]
    return ((2 + w / 16 + 0.11 * f) - 1j * (0.1 + w / 512 + 0.02 * f)).astype(np.complex64)


def permuted_upper(table):
    """``table`` with its entries of the last 64 indices (last axis) reversed: what a lookup at a wrong upper index would read."""
    out = np.array(table)
    out[..., -64:] = out[..., -64:][..., ::-1]
    return out


# ---- the geometry of every candidate, once per case --------------------------------------------------------------------------------
@contextlib.contextmanager
def shared_geometry(walls, fixed, X, Y, lo, hi, role, masked, mode_kw):
    """Inside the block ``R.accumulate_candidate`` answers from a table of ``(valid, pts, loss)`` computed side by side for the
    candidates of this case (the module's docstring says how and why); the path function is evaluated per call, as the loop does."""
    xp = R.NUMPY
    kw = dict(mode_kw)
    approx = kw.pop("approx")
    shape = np.shape(X)
    w = xp.asarray(walls)
    objs = [R.Obj(R.WALL, w[j]) for j in range(w.shape[0])]
    cells = R.vec(xp.asarray(X).reshape(-1), xp.asarray(Y).reshape(-1), xp)
    fx = xp.asarray(fixed)
    a, b = (fx, cells) if role == "rx" else (cells, fx)
    table = {}
    for k, cands in R.candidates_by_order(w.shape[0], lo, hi, None, set(masked) or None):
        if k == 0:
            continue  # the line of sight goes through the real function
        for at in range(0, len(cands), BATCH):
            part = cands[at:at + BATCH]
            inter = [R.Obj(R.WALL, w[part[:, i]][:, None]) for i in range(k)]
            pts, loss = R.image_path(a, inter, b, xp)
            on = R.on_objects(inter, pts, approx, xp=xp, **kw)
            hit = R.intersects_with_objects_batched(objs, part, pts, R.DEFAULT_PATCH, approx, xp=xp, **kw)
            ok = R.less(loss, xp.c(R.DEFAULT_TOL), approx, xp=xp, **kw)
            valid = xp.nan_to_num(R.logical_all([on, R.logical_not(hit, approx, xp=xp), ok], approx, xp=xp))
            full = [np.broadcast_to(np.asarray(p, F), (len(part), cells.shape[0], 2)) for p in pts]
            for row, cand in enumerate(part):
                table[tuple(int(o) for o in cand)] = (valid[row].reshape(shape), [p[row].reshape(shape + (2,)) for p in full],
                                                      np.broadcast_to(loss[row], cells.shape[:1]).reshape(shape))
    real = R.accumulate_candidate

    def served(tx, scene_objs, cand, rx, fun="received_power", fun_kwargs=None, solver="image", approx_=False, xp_=R.NUMPY, **kw_):
        assert solver == "image" and approx_ == approx and kw_ == kw and len(scene_objs) == len(objs), (solver, approx_, kw_)
        if len(cand) == 0:
            return real(tx, scene_objs, cand, rx, fun, fun_kwargs, solver, approx_, xp_, **kw_)
        valid, pts, loss = table[tuple(int(o) for o in cand)]
        f = R.FUNS[fun] if isinstance(fun, str) else fun
        return valid, f(pts, xp=xp_, **(fun_kwargs or {})), pts, loss

    R.accumulate_candidate = served
    try:
        yield
    finally:
        R.accumulate_candidate = real


PROFILE = (0.0, 3.0, 24)  # r_min, r_max, nbins of the power-delay profile: the longest double reflections overshoot

Inputs = namedtuple("Inputs", "cands T Rl total D S Sc Tc totalc totalp profile seconds")


def gather(walls, fixed, X, Y, lo, hi, role, masked, mode_kw, coef):
    """``Inputs``: what the products' folds take, each from the oracle that defines it -- ``contributions`` (``T``, ``Rl``, ``total``
    of received_power with ``FUN_KW``; ``Tc``, ``totalc`` of received_power_per_object with ``coef``), ``directed_contributions``
    (``D``), ``segment_contributions`` (``S``), ``scale_contributions`` (``Sc``), ``profile_map`` (``profile``, over ``PROFILE``)
    and ``coef_map`` (which has to agree with ``totalc``; ``totalp`` is the same map with the upper 64 coefficients permuted) -- all
    read-only, over one shared geometry."""
    from field_coefs_vjp_oracle import scale_contributions
    from object_coefs_oracle import coef_map
    from power_profile_oracle import profile_map
    from material_response_oracle import segment_contributions
    from power_angle_oracle import directed_contributions
    from strongest_paths_oracle import contributions

    t0 = time.perf_counter()
    kw = dict(min_order=lo, max_order=hi, grid_role=role, filter_nodes=set(masked) or None, **mode_kw)
    with shared_geometry(walls, fixed, X, Y, lo, hi, role, masked, mode_kw):
        cands, T, Rl, total = contributions(walls, fixed, X, Y, fun="received_power", fun_kwargs=FUN_KW, **kw)
        cands2, T2, D = directed_contributions(walls, fixed, X, Y, fun="received_power", fun_kwargs=FUN_KW, **kw)
        cands3, T3, Rl3, S = segment_contributions(walls, fixed, X, Y, fun="received_power", fun_kwargs=FUN_KW, **kw)
        cands4, Sc, Rl4 = scale_contributions(walls, fixed, X, Y, HEIGHT, **kw)
        _, Tc, Rl5, totalc = contributions(walls, fixed, X, Y, fun="received_power_per_object", coef=coef, fun_kwargs=dict(height=HEIGHT), **kw)
        profile = profile_map(walls, fixed, X, Y, *PROFILE, fun="received_power", fun_kwargs=FUN_KW, **kw)
        cmap = coef_map(walls, coef, fixed, X, Y, height=HEIGHT, **kw)
        totalp = coef_map(walls, permuted_upper(coef), fixed, X, Y, height=HEIGHT, **kw)
    bits = lambda x: x.view(np.uint32)  # noqa: E731
    for other in (cands2, cands3, cands4):
        assert len(other) == len(cands) and all(np.array_equal(p, q) for p, q in zip(cands, other))
    assert np.array_equal(bits(T), bits(T2)) and np.array_equal(bits(T), bits(T3))
    assert all(np.array_equal(bits(Rl), bits(r)) for r in (Rl3, Rl4, Rl5))
    assert np.array_equal(bits(np.ascontiguousarray(cmap, F)).reshape(-1), bits(totalc))
    totalp = np.ascontiguousarray(np.broadcast_to(totalp, np.shape(X)), F).reshape(-1)
    out = Inputs(cands, T, Rl, total, D, S, Sc, Tc, totalc, totalp, profile, time.perf_counter() - t0)
    for x in out[1:-1]:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def inputs_of(name, mode, role):
    """The ``Inputs`` of a case in one mode and role: computed once per session and shared among all products."""
    c = CASES[name]
    return gather(*scene_of(name), c.lo, c.hi, role, c.masked, MODES[mode], coefs_of(name))


# ---- what must hold of the oracle before any comparison ---------------------------------------------------------------------------
def conditions(name, mode, role):
    """The conditions every case has to meet on the oracle alone, so that no comparison passes on empty ground; returns the figures
    for printing."""
    c = CASES[name]
    inp = inputs_of(name, mode, role)
    cands, T = inp.cands, inp.T
    live = ~(T == 0)
    contributing = [tuple(int(o) for o in cand) for cand, z in zip(cands, live.any(axis=1)) if z]
    upper = [cand for cand in contributing if any(o >= 64 for o in cand)]
    assert len(upper) >= 20, (name, mode, role, len(upper))
    lit = live.any(axis=0).mean()
    assert lit > 1 / 3, (name, mode, role, lit)
    figures = dict(candidates=len(cands), contributing=len(contributing), upper=len(upper), lit=round(float(lit), 2))
    if name == "random260_o2":
        first, second = sum(cand[0] >= 64 for cand in contributing), sum(cand[1] >= 64 for cand in contributing)
        assert first >= 5 and second >= 5, (first, second)
        chunks = {o >> 6 for cand in contributing for o in cand}
        assert chunks == {0, 1, 2, 3, 4}, chunks
        figures.update(first=first, second=second)
    if c.n > 256:
        beyond = sum(any(o >= 256 for o in cand) for cand in contributing)
        assert beyond >= 1, (name, beyond)
        figures.update(beyond256=beyond)
    if c.masked:
        assert not any(o in c.masked for cand in cands for o in cand)
        assert sum(o < 64 for o in c.masked) >= 3
    if c.lo > 0:
        assert min(len(cand) for cand in cands) == c.lo
    # the per-wall coefficients: the negative wall's contributions are negative somewhere, the zero wall's contributions vanish
    neg, zero = SPECIAL_WALLS[name][:2]
    through = lambda w: np.array([w in cand for cand in cands])  # noqa: E731
    assert (inp.Tc[through(neg)] < 0).any(), (name, neg)
    assert live[through(zero)].any() and not inp.Tc[through(zero)].any(), (name, zero)
    for w in SPECIAL_WALLS[name][2:]:
        assert live[through(w)].any(), (name, w)
    # ... and a lookup at a wrong upper index changes bits
    assert (inp.totalp.view(np.uint32) != inp.totalc.view(np.uint32)).any(), name
    return figures
