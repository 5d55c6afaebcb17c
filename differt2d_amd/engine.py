"""
Thin object wrapper over the C ABI: one :class:`Context` = one MI355X + one HIP stream.

The higher-level mirror of the reference API (:mod:`differt2d_amd.scene`) drives this class;
benchmarks and tests may use it directly.
"""

from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _lib as L
from .defaults import DEFAULT_ALPHA, DEFAULT_HEIGHT, DEFAULT_PATCH, DEFAULT_R_COEF

FUN_IDS = {
    "received_power": L.FUN_RECEIVED_POWER,
    "length_squared": L.FUN_LENGTH_SQUARED,
    "length": L.FUN_LENGTH,
    "one": L.FUN_ONE,
    "received_power_per_object": L.FUN_RECEIVED_POWER_PER_OBJECT,  # one coefficient per object: Context.set_reflection_coefs
    "custom": L.FUN_CUSTOM,  # values and derivatives from the host: Context.set_path_fun_values (value+grad launches only)
}
ACT_IDS = {"hard_sigmoid": L.ACT_HARD_SIGMOID, "sigmoid": L.ACT_SIGMOID}
SOLVER_IDS = {"image": L.SOLVER_IMAGE, "min": L.SOLVER_MINPATH, "fermat": L.SOLVER_FERMAT}


def make_params(
    min_order: int = 0,
    max_order: int = 1,
    order: Optional[int] = None,
    approx: bool = False,
    function: str = "hard_sigmoid",
    alpha: float = DEFAULT_ALPHA,
    tol: float = 1e-2,
    patch: float = DEFAULT_PATCH,
    seg_tol: float = 0.005,
    fun: str = "received_power",
    r_coef: float = DEFAULT_R_COEF,
    height: float = DEFAULT_HEIGHT,
    solver: str = "image",
    steps: int = 100,
    out_mode: int = L.OUT_OVERWRITE,
    grid_role: int = L.GRID_RX,
    strict_nan: bool = False,
    many: int = 1,
) -> L.Params:
    """Builds a ``d2d_params``; keyword names follow the reference's kwargs
    (scene.py:1803-1826, geometry.py:910-919, logic.py:258-267, utils.py:17-24)."""
    if order is not None:
        min_order = max_order = order
    if function not in ACT_IDS:
        raise L.D2DUnsupported(-4, f"activation {function!r} is not native (hard_sigmoid, sigmoid)")
    if fun not in FUN_IDS:
        raise L.D2DUnsupported(-4, f"path function {fun!r} is not native ({', '.join(FUN_IDS)})")
    p = L.Params()
    p.min_order, p.max_order = int(min_order), int(max_order)
    p.approx, p.act = int(bool(approx)), ACT_IDS[function]
    p.alpha, p.tol, p.patch, p.seg_tol = float(alpha), float(tol), float(patch), float(seg_tol)
    p.fun_id, p.r_coef, p.height = FUN_IDS[fun], float(r_coef), float(height)
    p.solver, p.steps, p.out_mode = SOLVER_IDS[solver], int(steps), int(out_mode)
    p.grid_role = int(grid_role)
    p.strict_nan = int(bool(strict_nan))
    p.many = int(many)
    return p


class StrongestPaths(NamedTuple):
    """Result of :meth:`Context.strongest_paths` (include/d2d.h: d2d_strongest_paths_launch): slots first, cell axes after."""

    power: np.ndarray   # fp32 [k, m, n]: the slot's contribution valid * fun (+0.0: empty)
    length: np.ndarray  # fp32 [k, m, n]: the slot's path length (NaN: empty)
    cand: np.ndarray    # int32 [k, m, n, D2D_MAX_ORDER]: wall indices of the path, -1 padded
    order: np.ndarray   # int32 [k, m, n]: order of the path (-1: empty)
    total: np.ndarray   # fp32 [m, n]: the sum over all candidates, the fused map bit for bit
    count: np.ndarray   # int32 [m, n]: non-zero contributions of the cell


class CoherentField(NamedTuple):
    """Result of :meth:`Context.coherent_field` (include/d2d.h: d2d_coherent_field_launch)."""

    re: np.ndarray     # fp32 [m, n]: real part of the sum of a * e^(-j 2 pi r / lambda)
    im: np.ndarray     # fp32 [m, n]: imaginary part
    total: np.ndarray  # fp32 [m, n]: the incoherent sum over all candidates, the fused map bit for bit


class FrequencyResponse(NamedTuple):
    """Result of :meth:`Context.frequency_response` (include/d2d.h: d2d_frequency_response_launch)."""

    re: np.ndarray     # fp32 [nf, m, n]: real part of the sum of a * e^(-j 2 pi r * inv_wavelength[j])
    im: np.ndarray     # fp32 [nf, m, n]: imaginary part
    total: np.ndarray  # fp32 [m, n]: the incoherent sum over all candidates, the fused map bit for bit


class PositionGradient(NamedTuple):
    """Result of :meth:`Context.field_position_vjp` (include/d2d.h: d2d_field_position_vjp_launch)."""

    cell_bar: np.ndarray     # fp32 [m, n, 2]: dL / d (position of the cell): the receiver on an RX grid, the transmitter on a TX grid
    fixed_terms: np.ndarray  # fp32 [m, n, 2]: the cell's share of dL / d (fixed end point)
    fixed_bar: np.ndarray    # float64 [2]: dL / d (fixed end point), the fixed-order sum of fixed_terms over the cells


class WallGradient(NamedTuple):
    """Result of :meth:`Context.field_walls_vjp` (include/d2d.h: d2d_field_walls_vjp_launch)."""

    walls_bar: np.ndarray   # float64 [N, 2, 2]: dL / d (end point e of wall w), normal_bar[w, e] times the wall's fp32 unit normal
    normal_bar: np.ndarray  # float64 [N, 2]: the sensitivity of L to moving end point A or B of wall w along the wall's unit normal


class PowerAngleProfile(NamedTuple):
    """Result of :meth:`Context.power_angle` (include/d2d.h: d2d_power_angle_launch)."""

    bins: np.ndarray   # fp32 [nbins, m, n]: the contributions whose direction at the chosen end falls into the bin
    total: np.ndarray  # fp32 [m, n]: the sum over all candidates, the fused map bit for bit


class ArrayResponse(NamedTuple):
    """Result of :meth:`Context.array_response` (include/d2d.h: d2d_array_response_launch)."""

    re: np.ndarray     # fp32 [nr, nt, m, n]: real part of H[i, j], the coherent sum between transmit element j and receive element i
    im: np.ndarray     # fp32 [nr, nt, m, n]: imaginary part
    total: np.ndarray  # fp32 [m, n]: the incoherent sum over all candidates, the fused map bit for bit


class ArrayFrequencyResponse(NamedTuple):
    """Result of :meth:`Context.array_frequency_response` (include/d2d.h: d2d_array_frequency_response_launch)."""

    re: np.ndarray     # fp32 [nf, nr, nt, m, n]: real part of H[f, i, j], the array response's H[i, j] at inv_wavelengths[f]
    im: np.ndarray     # fp32 [nf, nr, nt, m, n]: imaginary part
    total: np.ndarray  # fp32 [m, n]: the incoherent sum over all candidates, the fused map bit for bit (None where not asked for)


class BeamResponse(NamedTuple):
    """Result of :meth:`Context.beam_response` (include/d2d.h: d2d_beam_response_launch)."""

    re: np.ndarray     # fp32 [nf, nbr, nbt, m, n]: real part of y[f, br, bt] = w_rx[br]^H H[f] w_tx[bt]
    im: np.ndarray     # fp32 [nf, nbr, nbt, m, n]: imaginary part
    total: np.ndarray  # fp32 [m, n]: the incoherent sum over all candidates, the fused map bit for bit (None where not asked for)


FIELD_AMPLITUDES = {"sqrt": L.D2D_FIELD_AMP_SQRT, "linear": L.D2D_FIELD_AMP_LINEAR}
ANGLE_ENDS = {"tx": L.D2D_ANGLE_AT_TX, "rx": L.D2D_ANGLE_AT_RX}
POLARIZATIONS = {"te": L.D2D_POL_TE, "tm": L.D2D_POL_TM}


def _amplitude_id(method: str, amplitude) -> int:
    """The library's constant of an amplitude mode that may be given by name; ``method`` begins the refusal of an unknown name."""
    if isinstance(amplitude, str):
        if amplitude not in FIELD_AMPLITUDES:
            raise L.D2DError(-1, f"{method}: amplitude must be one of {sorted(FIELD_AMPLITUDES)}, got {amplitude!r}")
        amplitude = FIELD_AMPLITUDES[amplitude]
    return int(amplitude)


def _polarization_id(method: str, polarization) -> int:
    """The library's constant of a polarisation that may be given by name; ``method`` begins the refusal of an unknown name."""
    if isinstance(polarization, str):
        if polarization.lower() not in POLARIZATIONS:
            raise L.D2DError(-1, f"{method}: polarization must be one of {sorted(POLARIZATIONS)}, got {polarization!r}")
        polarization = POLARIZATIONS[polarization.lower()]
    return int(polarization)


def _keep_pointer(a: np.ndarray, *shape) -> np.ndarray:
    """An empty list still hands the library a pointer: it refuses a count of 0 itself."""
    return a if a.size else np.zeros(shape, np.float32)


def _permittivity_table(method: str, permittivity, nf: int) -> np.ndarray:
    """The permittivities as contiguous complex64 ``[nf, N]``: ``[N]`` stands for equal rows; any other shape is refused here."""
    eps = np.asarray(permittivity)
    if eps.ndim == 1:
        eps = np.broadcast_to(eps, (max(nf, 1), eps.size))
    if eps.ndim != 2 or eps.shape[0] != max(nf, 1):
        raise L.D2DError(-1, f"{method}: permittivity must be complex [N] or [nf, N] with nf = {nf}, got shape {tuple(eps.shape)}")
    return np.ascontiguousarray(eps, dtype=np.complex64)


def _cotangent_planes(method: str, re_bar, im_bar, nf: int, shape, keep: np.ndarray):
    """The cotangents of a response's planes as contiguous fp32 ``[nf, m, n]``, refused here when either has another shape (without
    a grid, ``shape`` empty, the library refuses before it reads anything); an empty list hands the library ``keep`` in their place."""
    rb = np.ascontiguousarray(re_bar, dtype=np.float32)
    ib = np.ascontiguousarray(im_bar, dtype=np.float32)
    planes = (nf,) + tuple(shape or ())
    if nf and shape and (rb.shape != planes or ib.shape != planes):
        raise L.D2DError(-1, f"{method}: re_bar and im_bar must have the shape {planes} of the response's planes, got {rb.shape} and {ib.shape}")
    return (rb, ib) if nf else (keep, keep)


def _beam_weights(name: str, w, n: int) -> np.ndarray:
    """A codebook as contiguous complex64 ``[nb, n]``: ``[n]`` is one beam; any other shape is refused here (the library sees only
    counts).  An empty codebook stays empty: the library refuses a count of 0 itself."""
    w = np.asarray(w)
    if w.ndim == 1 and w.size:
        w = w.reshape(1, -1)
    if w.ndim != 2 or (w.size and w.shape[1] != n):
        raise L.D2DError(-1, f"beam_response: {name} must be complex [nb, {n}] (or [{n}] for one beam), got shape {tuple(w.shape)}")
    return np.ascontiguousarray(w, dtype=np.complex64).reshape(w.shape[0], n)


def _no_result(ctx, getter, launch_name: str, *nulls):
    """A getter without an accepted launch: the library says why (nothing is copied: ``nulls`` are its buffers)."""
    L.check(getter(ctx, *nulls))
    raise L.D2DError(-5, f"{launch_name} must come first")


def _immutable(a: np.ndarray) -> bool:
    """Nobody can write to this array's memory through NumPy: it and every array it is a view of are read-only."""
    while isinstance(a, np.ndarray):
        if a.flags.writeable:
            return False
        a = a.base
    return a is None


class Context:
    """Owns a ``d2d_ctx``: device buffers for one scene and one RX grid stay resident in HBM."""

    def __init__(self, device: int = 0):
        self._lib = L.load()
        self._ctx = C.c_void_p()
        L.check(self._lib.d2d_create(int(device), C.byref(self._ctx)))
        self.device = int(device)
        self.shape = None
        self.n_objects = 0
        self._grid_held = None
        self._grid_serial = 0
        self._top_k = 0  # slots per cell of the last launch_strongest_paths that was accepted
        self._field = False  # a launch_coherent_field was accepted
        self._freq_nf = 0  # planes of the last launch_frequency_response that was accepted
        self._angle_nbins = 0  # bins of the last launch_power_angle that was accepted
        self._array_shape = None  # (nr, nt) of the last launch_array_response that was accepted
        self._wide_shape = None  # (nf, nr, nt) of the last launch_array_frequency_response that was accepted
        self._beam_shape = None  # (nf, nbr, nbt) of the last launch_beam_response that was accepted
        self._mat_nf = 0  # planes of the last launch_material_response that was accepted
        self._eps_vjp_nf = 0  # rows of the last launch_material_eps_vjp that was accepted

    # -- lifetime ---------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.d2d_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, mem = C.c_int(0), C.c_int64(0)
        L.check(self._lib.d2d_device_info(self.device, name, 256, C.byref(cus), C.byref(mem)))
        return {"name": name.value.decode(), "cus": cus.value, "mem_bytes": mem.value}

    # -- scene ------------------------------------------------------------------------
    def set_scene(self, xys, kind=None, phi=None):
        xys = np.ascontiguousarray(xys, dtype=np.float32).reshape(-1, 2, 2)
        n = xys.shape[0]
        kind_a = None if kind is None else np.ascontiguousarray(kind, dtype=np.uint8)
        phi_a = None if phi is None else np.ascontiguousarray(phi, dtype=np.float32)
        if kind_a is not None and kind_a.shape != (n,):
            raise ValueError("kind must have one entry per object")
        if phi_a is not None and phi_a.shape != (n,):
            raise ValueError("phi must have one entry per object")
        L.check(
            self._lib.d2d_set_scene(
                self._ctx,
                xys.ctypes.data_as(C.c_void_p) if n else None,
                None if kind_a is None else kind_a.ctypes.data_as(C.c_void_p),
                None if phi_a is None else phi_a.ctypes.data_as(C.c_void_p),
                n,
            )
        )
        self.n_objects = n

    def set_candidate_mask(self, allowed=None):
        if allowed is None:
            L.check(self._lib.d2d_set_candidate_mask(self._ctx, None))
            return
        a = np.ascontiguousarray(allowed, dtype=np.uint8)
        if a.shape != (self.n_objects,):
            raise ValueError("mask must have one entry per object")
        L.check(self._lib.d2d_set_candidate_mask(self._ctx, a.ctypes.data_as(C.c_void_p)))

    def set_reflection_coefs(self, coefs=None):
        """One reflection coefficient per object of the resident scene, for ``fun="received_power_per_object"`` (include/d2d.h:
        d2d_set_reflection_coefs).  They stay with the scene: another scene drops them; ``None`` drops them too."""
        if coefs is None:
            L.check(self._lib.d2d_set_reflection_coefs(self._ctx, None, 0))
            return
        c = np.ascontiguousarray(coefs, dtype=np.float32).reshape(-1)
        L.check(self._lib.d2d_set_reflection_coefs(self._ctx, c.ctypes.data_as(C.c_void_p), c.size))

    def get_reflection_coefs_vjp(self) -> np.ndarray:
        """``<cotangent, d Z / d coefficients>`` [N] of the last scene-VJP sweep(s); zeros unless they ran
        ``fun="received_power_per_object"`` (include/d2d.h: d2d_get_reflection_coefs_vjp)."""
        out = np.zeros(max(self.n_objects, 1), np.float32)
        L.check(self._lib.d2d_get_reflection_coefs_vjp(self._ctx, out))
        return out[: self.n_objects]

    def num_candidates(self, min_order=0, max_order=1) -> int:
        n = C.c_int64(0)
        L.check(self._lib.d2d_num_candidates(self._ctx, min_order, max_order, C.byref(n)))
        return n.value

    def list_candidates(self, min_order=0, max_order=1):
        """Returns the reference's candidate list: a python list of int32 arrays of shape (k,)."""
        n = self.num_candidates(min_order, max_order)
        cand = np.empty((max(n, 1), L.D2D_MAX_ORDER), np.int32)
        order = np.empty(max(n, 1), np.int32)
        L.check(
            self._lib.d2d_list_candidates(
                self._ctx, min_order, max_order, cand.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p), n
            )
        )
        return [cand[i, : order[i]].copy() for i in range(n)]

    # -- grid sweep -------------------------------------------------------------------
    def set_grid(self, X, Y):
        """Makes (X, Y) the resident grid.  A grid that is resident already is recognised -- by identity when both arrays
        are immutable (read-only, like the reference's JAX arrays: no byte of them is read then), else byte for byte against
        the library's host copy of the resident arrays --
        and is not uploaded again; the schedule's work history and the regions' boxes stay valid (include/d2d.h)."""
        Xc = np.ascontiguousarray(X, dtype=np.float32)
        Yc = np.ascontiguousarray(Y, dtype=np.float32)
        if Xc.shape != Yc.shape or Xc.ndim != 2:
            raise ValueError(f"X and Y must be 2-D arrays of one shape, got {Xc.shape} and {Yc.shape}")
        token = 0
        if _immutable(Xc) and _immutable(Yc):
            held = self._grid_held
            if held is not None and held[0] is Xc and held[1] is Yc:
                token = held[2]
            else:
                self._grid_serial += 1
                token = self._grid_serial
                self._grid_held = (Xc, Yc, token)  # (keeps the arrays alive: their identity stays theirs)
            L.check(self._lib.d2d_set_grid_versioned(self._ctx, Xc, Yc, Xc.shape[0], Xc.shape[1], token))
        else:
            self._grid_held = None
            L.check(self._lib.d2d_set_grid(self._ctx, Xc, Yc, Xc.shape[0], Xc.shape[1]))
        self.shape = Xc.shape

    def grid_reuses(self) -> int:
        """Diagnostic: set_grid calls that found their grid resident already."""
        n = C.c_int64(0)
        L.check(self._lib.d2d_debug_grid_reuses(self._ctx, C.byref(n)))
        return int(n.value)

    def sweep_shape(self) -> tuple:
        """Diagnostic: (waves per patch, shared candidate by candidate?) of the last RX-grid value sweep (include/d2d.h)."""
        w, k = C.c_int32(0), C.c_int32(0)
        L.check(self._lib.d2d_debug_sweep_shape(self._ctx, C.byref(w), C.byref(k)))
        return int(w.value), bool(k.value)

    def txg_fallbacks(self) -> int:
        """Diagnostic: TX-grid sweeps that ran exhaustively because a degenerate path is not exactly invalid under their
        tol / alpha / activation (include/d2d.h, d2d_params.grid_role)."""
        n = C.c_int64(0)
        L.check(self._lib.d2d_debug_txg_fallbacks(self._ctx, C.byref(n)))
        return int(n.value)

    def hidden_masks(self) -> tuple:
        """Diagnostic: (times the last-segment masks were built, valid now?) (include/d2d.h)."""
        n, v = C.c_int64(0), C.c_int32(0)
        L.check(self._lib.d2d_debug_hidden_masks(self._ctx, C.byref(n), C.byref(v)))
        return int(n.value), bool(v.value)

    def launch(self, params: L.Params, tx):
        tx = np.ascontiguousarray(tx, dtype=np.float32).reshape(2)
        L.check(self._lib.d2d_power_map_launch(self._ctx, C.byref(params), tx))

    def set_cotangent(self, cot=None):
        """Cotangent of the value map for the scene VJP (None = ones)."""
        if cot is None:
            L.check(self._lib.d2d_set_cotangent(self._ctx, None))
            return
        cot = np.ascontiguousarray(cot, dtype=np.float32)
        if cot.shape != self.shape:
            raise ValueError(f"cotangent must have the grid's shape {self.shape}, got {cot.shape}")
        L.check(self._lib.d2d_set_cotangent(self._ctx, cot.ctypes.data_as(C.c_void_p)))

    def set_path_fun_values(self, f=None, xys_bar=None):
        """A host-evaluated path function for ``launch_vg(make_params(fun="custom", ...))``: ``f`` [C, m, n] and its derivative
        w.r.t. the path points ``xys_bar`` [C, m, n, D2D_MAX_ORDER + 2, 2], candidates in the sweep's order (include/d2d.h)."""
        if f is None:
            L.check(self._lib.d2d_set_path_fun_values(self._ctx, None, None, 0))
            return
        f = np.ascontiguousarray(f, dtype=np.float32)
        xys_bar = np.ascontiguousarray(xys_bar, dtype=np.float32)
        if f.ndim != 3 or f.shape[1:] != self.shape or xys_bar.shape != f.shape + (L.D2D_MAX_ORDER + 2, 2):
            raise ValueError(f"f must be [C, {self.shape[0]}, {self.shape[1]}] and xys_bar f.shape + ({L.D2D_MAX_ORDER + 2}, 2); "
                             f"got {f.shape} and {xys_bar.shape}")
        L.check(self._lib.d2d_set_path_fun_values(self._ctx, f.ctypes.data_as(C.c_void_p), xys_bar.ctypes.data_as(C.c_void_p), f.shape[0]))

    def launch_vg(self, params: L.Params, tx, scene_vjp: bool = False):
        """Fused value+grad sweep (per-cell d/d rx; optionally the VJP w.r.t. tx and object end points)."""
        tx = np.ascontiguousarray(tx, dtype=np.float32).reshape(2)
        L.check(self._lib.d2d_power_map_vg_launch(self._ctx, C.byref(params), tx, int(bool(scene_vjp))))

    def get_grad_rx(self) -> np.ndarray:
        out = np.empty((*self.shape, 2), np.float32)
        L.check(self._lib.d2d_get_grad_rx(self._ctx, out.reshape(-1)))
        return out

    def get_scene_vjp(self, with_phi: bool = False):
        """Returns (tx_bar[2], xys_bar[N,2,2]) -- and phi_bar[N] (RIS angles) with ``with_phi``."""
        tx_bar = np.zeros(2, np.float32)
        xys_bar = np.zeros((max(self.n_objects, 1), 2, 2), np.float32)
        phi_bar = np.zeros(max(self.n_objects, 1), np.float32)
        L.check(self._lib.d2d_get_scene_vjp(self._ctx, tx_bar, xys_bar.ctypes.data_as(C.c_void_p),
                                            phi_bar.ctypes.data_as(C.c_void_p) if with_phi else None))
        if with_phi:
            return tx_bar, xys_bar[: self.n_objects], phi_bar[: self.n_objects]
        return tx_bar, xys_bar[: self.n_objects]

    def value_and_grads(self, tx, X, Y, cotangent=None, **kw):
        """One call: value map, per-cell grad_rx, tx_bar, walls_bar (mirrors oracle.ref.power_map_value_and_grads)."""
        self.set_grid(X, Y)
        self.set_cotangent(cotangent)
        self.launch_vg(make_params(**kw), tx, scene_vjp=True)
        value = self.get_map()
        tx_bar, walls_bar, phi_bar = self.get_scene_vjp(with_phi=True)
        return {"value": value, "grad_rx": self.get_grad_rx(), "tx_bar": tx_bar, "walls_bar": walls_bar, "phi_bar": phi_bar}

    def launch_stats(self, params: L.Params, tx) -> np.ndarray:
        """Runs the instrumented kernel build; returns the executed-work counters (include/d2d.h)."""
        tx = np.ascontiguousarray(tx, dtype=np.float32).reshape(2)
        stats = np.zeros(L.D2D_NUM_STATS, np.uint64)
        L.check(self._lib.d2d_power_map_stats(self._ctx, C.byref(params), tx, stats))
        return stats

    def set_option(self, name: str, value: int) -> None:
        """Launch-shape tuning (``split_max_tiles``, ``sched_min_tiles``): changes speed, never a result bit."""
        L.check(self._lib.d2d_set_option(self._ctx, name.encode(), int(value)))

    def debug_set_schedule(self, order=None) -> None:
        """Diagnostic: later launches of ``len(order)`` patches start their patches in this order (None: built-in)."""
        if order is None:
            L.check(self._lib.d2d_debug_set_schedule(self._ctx, np.zeros(1, np.int32), 0))
        else:
            o = np.ascontiguousarray(order, dtype=np.int32)
            L.check(self._lib.d2d_debug_set_schedule(self._ctx, o, o.size))

    def debug_get_schedule(self, n_patches: int):
        """Diagnostic: (order, cost keys) of the schedule built by the last scheduled launch."""
        order, key = np.empty(n_patches, np.int32), np.empty(n_patches, np.uint8)
        L.check(self._lib.d2d_debug_get_schedule(self._ctx, order, key, n_patches))
        return order, key

    def debug_get_work(self, n_patches: int) -> np.ndarray:
        """Diagnostic: the work (units of ~25 wave-instructions) each patch took in the last culled sweep."""
        out = np.empty(n_patches, np.uint32)
        L.check(self._lib.d2d_debug_get_work(self._ctx, out, n_patches))
        return out

    def debug_region_stats(self) -> dict:
        """Diagnostic: the region candidate lists of the last launch that built any (include/d2d.h)."""
        o = np.zeros(8, np.int64)
        L.check(self._lib.d2d_debug_region_stats(self._ctx, o))
        return {"pool_chunks_used": int(o[0]), "pool_chunks": int(o[1]), "patches_enumerated": int(o[2]), "regions_not_listed": int(o[3]),
                "leaf_entries": {2: int(o[4]), 3: int(o[5]), 4: int(o[6])}, "leaf_regions": int(o[7])}

    def debug_nan_scan(self) -> dict:
        """Diagnostic: counters of the last value+grad launch's NaN scan (needs ``set_option("nan_scan_stats", 1)``)."""
        o = np.zeros(6, np.int64)
        L.check(self._lib.d2d_debug_nan_scan(self._ctx, o))
        return {"probes": int(o[0]), "nan_cells": int(o[1]), "nan_patches": int(o[2]), "self_probes": int(o[3]), "bad_items": int(o[4]),
                "rounds": int(o[5])}

    def last_kernel_ms(self) -> float:
        """Duration of the sweep kernel of the last launch (needs ``set_option("time_kernel", 1)``)."""
        ms = C.c_float(0.0)
        L.check(self._lib.d2d_last_kernel_ms(self._ctx, C.byref(ms)))
        return float(ms.value)

    def wave_cycles(self, params: L.Params, tx) -> np.ndarray:
        """Shader-clock ticks per wave (8 x 8 patch) of the instrumented forward sweep, shape (patch rows, patch cols)."""
        tx = np.ascontiguousarray(tx, dtype=np.float32).reshape(2)
        ty, tx_ = -(-self.shape[0] // 8), -(-self.shape[1] // 8)
        out = np.zeros(ty * tx_, np.uint64)
        n = C.c_int64(0)
        L.check(self._lib.d2d_power_map_wave_cycles(self._ctx, C.byref(params), tx, out, out.size, C.byref(n)))
        return out.reshape(ty, tx_)

    def selftest_div(self, x, y):
        """(q_fast, q_ref, q_hostr) of the division self-test (include/d2d.h)."""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
        outs = [np.empty_like(x) for _ in range(3)]
        L.check(self._lib.d2d_selftest_div(self._ctx, x, y, x.size, *outs))
        return outs

    def selftest_expf(self, x) -> np.ndarray:
        """The device's expf of the sigmoid activation (include/d2d.h: must equal the host libm's bit for bit)."""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        y = np.empty_like(x)
        L.check(self._lib.d2d_selftest_expf(self._ctx, x, x.size, y))
        return y

    def selftest_phasor(self, f):
        """``(cos(2 pi f), sin(2 pi f))`` as the coherent field's phasor computes them on the device (include/d2d.h: must equal the
        host build of d2d_phasor.hpp bit for bit); ``f`` in turns, in [0, 1)."""
        f = np.ascontiguousarray(f, dtype=np.float32).reshape(-1)
        c, s = np.empty_like(f), np.empty_like(f)
        L.check(self._lib.d2d_selftest_phasor(self._ctx, f, f.size, c, s))
        return c, s

    def selftest_angle(self, dx, dy):
        """``turns(dx, dy)``, the angle of the vectors in turns in [0, 1), as the power-angle profile computes it on the device
        (include/d2d.h: must equal the host build of d2d_angle.hpp bit for bit)."""
        dx = np.ascontiguousarray(dx, dtype=np.float32).reshape(-1)
        dy = np.ascontiguousarray(dy, dtype=np.float32).reshape(-1)
        if dx.size != dy.size:
            raise ValueError("dx and dy must have one size")
        out = np.empty_like(dx)
        L.check(self._lib.d2d_selftest_angle(self._ctx, dx, dy, dx.size, out))
        return out

    def selftest_steer(self, dx, dy, f0, qt, qr, inv):
        """``unit_dir(dx, dy)`` and ``steer_phase(f0, qt, qr, inv)`` as the array response computes them on the device
        (include/d2d.h: must equal the host build of d2d_steer.hpp bit for bit).  Returns ``(ux, uy, ok, f)``, ``ok`` as bool."""
        a = [np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in (dx, dy, f0, qt, qr, inv)]
        if any(v.size != a[0].size for v in a):
            raise ValueError("the six inputs must have one size")
        ux, uy, ok, f = (np.empty_like(a[0]) for _ in range(4))
        L.check(self._lib.d2d_selftest_steer(self._ctx, *a, a[0].size, ux, uy, ok, f))
        return ux, uy, ok != 0.0, f

    def selftest_fresnel(self, er, ei, c, polarization="te"):
        """``fresnel(er, ei, c, polarization)`` as the material response computes it on the device (include/d2d.h: must equal the
        host build of d2d_fresnel.hpp bit for bit).  Returns ``(gr, gi)``."""
        a = [np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in (er, ei, c)]
        if any(v.size != a[0].size for v in a):
            raise ValueError("the three inputs must have one size")
        gr, gi = np.empty_like(a[0]), np.empty_like(a[0])
        L.check(self._lib.d2d_selftest_fresnel(self._ctx, *a, _polarization_id("selftest_fresnel", polarization), a[0].size, gr, gi))
        return gr, gi

    def selftest_fresnel_grad(self, er, ei, c, polarization="te"):
        """``fresnel_grad(er, ei, c, polarization)`` as the permittivity adjoint computes it on the device (include/d2d.h: must
        equal the host build of d2d_fresnel_grad.hpp bit for bit).  Returns ``(gr, gi, dr, di, ok)``, ``ok`` as bool."""
        a = [np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in (er, ei, c)]
        if any(v.size != a[0].size for v in a):
            raise ValueError("the three inputs must have one size")
        gr, gi, dr, di, ok = (np.empty_like(a[0]) for _ in range(5))
        L.check(self._lib.d2d_selftest_fresnel_grad(self._ctx, *a, _polarization_id("selftest_fresnel_grad", polarization), a[0].size, gr, gi, dr, di, ok))
        return gr, gi, dr, di, ok != 0.0

    def get_map(self) -> np.ndarray:
        out = np.empty(self.shape, np.float32)
        L.check(self._lib.d2d_get_map(self._ctx, out))
        return out

    def synchronize(self):
        L.check(self._lib.d2d_synchronize(self._ctx))

    def power_map(self, tx, X, Y, **kw) -> np.ndarray:
        """One transmitter, one grid: upload, sweep, download."""
        self.set_grid(X, Y)
        self.launch(make_params(**kw), tx)
        return self.get_map()

    # -- individual paths -------------------------------------------------------------
    def set_theta0(self, theta0):
        """Initial guesses ``[C, <=D2D_MAX_ORDER]`` of the MinPath / FermatPath solvers for the next sweeps."""
        t = np.zeros((len(theta0), L.D2D_MAX_ORDER), np.float32)
        for i, row in enumerate(theta0):
            row = np.asarray(row, np.float32).reshape(-1)
            t[i, : row.size] = row
        L.check(self._lib.d2d_set_theta0(self._ctx, t.ctypes.data_as(C.c_void_p) if t.size else None, t.shape[0]))

    def set_optimizer(self, optimizer=None):
        """The optimiser of the MinPath / FermatPath solvers for the next sweeps (include/d2d.h: d2d_set_optimizer).  ``None`` =
        the reference's default, ``optax.adam(0.1)``; else an :class:`differt2d_amd.optimize.Adam` or
        :class:`differt2d_amd.optimize.SGD`."""
        from .optimize import SGD, Adam, default_optimizer

        o = default_optimizer() if optimizer is None else optimizer
        if isinstance(o, SGD):
            if o.momentum is None:
                L.check(self._lib.d2d_set_optimizer(self._ctx, L.D2D_OPT_SGD, float(o.learning_rate), 0.0, 0.0, 0.0))
            else:  # b1 = momentum, b2 = Nesterov flag
                nesterov = 1.0 if o.nesterov else 0.0
                L.check(self._lib.d2d_set_optimizer(self._ctx, L.D2D_OPT_SGD_MOMENTUM, float(o.learning_rate), float(o.momentum), nesterov, 0.0))
            return
        if not isinstance(o, Adam):
            raise L.D2DUnsupported(-4, f"optimizer {optimizer!r} is not native: differt2d_amd.optimize.adam(learning_rate, b1, b2, eps) is")
        L.check(self._lib.d2d_set_optimizer(self._ctx, L.D2D_OPT_ADAM, float(o.learning_rate), float(o.b1), float(o.b2), float(o.eps)))

    def trace_paths(self, params: L.Params, tx, rx, candidates, xys_in=None, loss_in=None, theta0=None):
        """Solves (or validates ``xys_in``) every candidate for every (tx, rx) pair on the GPU.

        ``tx``/``rx``: (P, 2); ``candidates``: list of int arrays. Returns a dict of arrays with leading
        shape (P, C): ``xys`` (P, C, D2D_MAX_ORDER+2, 2), ``loss``, ``valid``, ``on``, ``hit``, ``length``."""
        tx = np.ascontiguousarray(tx, dtype=np.float32).reshape(-1, 2)
        rx = np.ascontiguousarray(rx, dtype=np.float32).reshape(-1, 2)
        if tx.shape != rx.shape:
            raise ValueError("tx and rx must pair up")
        P, Cn = tx.shape[0], len(candidates)
        cand = np.full((max(Cn, 1), L.D2D_MAX_ORDER), -1, np.int32)
        order = np.zeros(max(Cn, 1), np.int32)
        for i, c in enumerate(candidates):
            c = np.asarray(c, dtype=np.int32).reshape(-1)
            if c.size > L.D2D_MAX_ORDER:
                raise L.D2DError(-1, f"candidate order {c.size} exceeds D2D_MAX_ORDER={L.D2D_MAX_ORDER}")
            cand[i, : c.size] = c
            order[i] = c.size
        NP = L.D2D_MAX_ORDER + 2
        out = {
            "xys": np.full((P, Cn, NP, 2), np.nan, np.float32),
            "loss": np.zeros((P, Cn), np.float32),
            "valid": np.zeros((P, Cn), np.float32),
            "on": np.zeros((P, Cn), np.float32),
            "hit": np.zeros((P, Cn), np.float32),
            "length": np.zeros((P, Cn), np.float32),
        }
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        if xys_in is not None:
            xys_in = np.ascontiguousarray(xys_in, dtype=np.float32).reshape(P, Cn, NP, 2)
        if loss_in is not None:
            loss_in = np.ascontiguousarray(loss_in, dtype=np.float32).reshape(P, Cn)
        th = None
        if theta0 is not None:
            # the library reads C * max(1, many) rows from this pointer: a shorter array would be a host out-of-bounds read
            need = Cn * max(1, int(params.many))
            if params.solver != L.SOLVER_IMAGE and xys_in is None and len(theta0) != need:
                raise ValueError(f"theta0 must have {need} rows (candidates x max(1, many)), got {len(theta0)}")
            th = np.zeros((max(len(theta0), 1), L.D2D_MAX_ORDER), np.float32)
            for i, row in enumerate(theta0):
                row = np.asarray(row, np.float32).reshape(-1)
                th[i, : row.size] = row
        L.check(
            self._lib.d2d_trace_paths(
                self._ctx, C.byref(params), tx, rx, P, cand, order, Cn, vp(th), 0 if theta0 is None else len(theta0),
                vp(xys_in), vp(loss_in),
                out["xys"].reshape(-1), out["loss"].reshape(-1), out["valid"].reshape(-1),
                vp(out["on"]), vp(out["hit"]), vp(out["length"]),
            )
        )
        out["order"] = order[:Cn]
        return out

    def valid_paths(self, params: L.Params, fixed) -> dict:
        """Every (cell of the resident grid, candidate of the current scene and mask) whose validity is not exactly zero, with
        its solved path: the record launch of the culled sweep (include/d2d.h: d2d_valid_paths; ImagePath, hard or
        hard_sigmoid validity).  ``params.grid_role`` says which end of the paths the cells are, ``fixed`` is the other end.

        Returns a dict of arrays with leading length n (record order unspecified): ``cell`` (row-major index into the grid),
        ``cand`` (n, D2D_MAX_ORDER; -1 padded), ``order``, ``xys`` (n, D2D_MAX_ORDER+2, 2; unused rows NaN), ``loss``,
        ``valid``, ``length`` -- the entries :meth:`trace_paths` returns for the same (pair, candidate), bit for bit."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        n = C.c_int64(0)
        L.check(self._lib.d2d_valid_paths(self._ctx, C.byref(params), fixed, C.byref(n)))
        n = int(n.value)
        out = {
            "cell": np.empty(n, np.int32),
            "cand": np.empty((n, L.D2D_MAX_ORDER), np.int32),
            "order": np.empty(n, np.int32),
            "xys": np.empty((n, L.D2D_MAX_ORDER + 2, 2), np.float32),
            "loss": np.empty(n, np.float32),
            "valid": np.empty(n, np.float32),
            "length": np.empty(n, np.float32),
        }
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        L.check(self._lib.d2d_get_valid_paths(self._ctx, n, vp(out["cell"]), vp(out["cand"]), vp(out["order"]), vp(out["xys"]),
                                              vp(out["loss"]), vp(out["valid"]), vp(out["length"])))
        return out

    def valid_paths_ms(self) -> dict:
        """Diagnostic: kernel times of the last :meth:`valid_paths` that found records (needs ``set_option("time_kernel", 1)``)."""
        ms = np.zeros(3, np.float32)
        L.check(self._lib.d2d_debug_valid_paths_ms(self._ctx, ms))
        return {"count_ms": float(ms[0]), "write_ms": float(ms[1]), "trace_ms": float(ms[2])}

    def power_profile(self, params: L.Params, fixed, r_min: float, r_max: float, nbins: int) -> np.ndarray:
        """Per-cell power-delay profile of the resident grid: the fused sweep's contributions ``valid * fun`` binned by path
        length into ``nbins`` half-open bins of equal width over ``[r_min, r_max)`` -- one launch of the bin build of the culled
        sweep (include/d2d.h: d2d_power_profile_launch holds the definition; ImagePath, hard or hard_sigmoid validity, every fused
        function).  ``params.grid_role`` says which end of the paths the cells are, ``fixed`` is the other end.  The resident value
        map is not touched.  Returns an fp32 array ``[nbins, m, n]``; :func:`differt2d_amd.utils.delay_statistics` reduces it."""
        self.launch_profile(params, fixed, r_min, r_max, nbins)
        return self.get_profile(nbins)

    def launch_profile(self, params: L.Params, fixed, r_min: float, r_max: float, nbins: int):
        """The launch of :meth:`power_profile` alone (asynchronous, like :meth:`launch`)."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        L.check(self._lib.d2d_power_profile_launch(self._ctx, C.byref(params), fixed, float(r_min), float(r_max), int(nbins)))

    def get_profile(self, nbins: int) -> np.ndarray:
        """Synchronises and returns the profile of the last :meth:`launch_profile`, which was launched with ``nbins`` bins."""
        out = np.empty((int(nbins),) + tuple(self.shape), np.float32)
        L.check(self._lib.d2d_get_power_profile(self._ctx, out))
        return out

    def strongest_paths(self, params: L.Params, fixed, k: int) -> "StrongestPaths":
        """The ``k`` strongest multipath components of every cell of the resident grid (``1 <= k <= D2D_TOP_MAX``): the fused
        sweep's contributions ``valid * fun`` with the largest magnitude, strongest first, ties in enumeration order -- one launch
        of the top-k build of the culled sweep (include/d2d.h: d2d_strongest_paths_launch holds the definition; ImagePath, hard or
        hard_sigmoid validity, every fused function).  ``params.grid_role`` says which end of the paths the cells are, ``fixed`` is
        the other end.  The resident value map, the records of :meth:`valid_paths` and the profile are not touched.

        Returns a :class:`StrongestPaths`: ``power`` and ``length`` fp32 ``[k, m, n]``, ``cand`` int32 ``[k, m, n, D2D_MAX_ORDER]``
        (-1 padded), ``order`` int32 ``[k, m, n]``, ``total`` fp32 ``[m, n]`` (the fused map, bit for bit) and ``count`` int32
        ``[m, n]`` (non-zero contributions; ``count > k``: something was cut).  An empty slot holds power +0.0, length NaN, order
        -1.  :func:`differt2d_amd.utils.strongest_share` gives the kept slots' share of ``total``."""
        self.launch_strongest_paths(params, fixed, k)
        return self.get_strongest_paths()

    def launch_strongest_paths(self, params: L.Params, fixed, k: int):
        """The launch of :meth:`strongest_paths` alone (asynchronous, like :meth:`launch`)."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        self._top_k = 0
        L.check(self._lib.d2d_strongest_paths_launch(self._ctx, C.byref(params), fixed, int(k)))
        self._top_k = int(k)

    def get_strongest_paths(self) -> "StrongestPaths":
        """Synchronises and returns the result of the last :meth:`launch_strongest_paths`."""
        k = self._top_k
        if k < 1:
            _no_result(self._ctx, self._lib.d2d_get_strongest_paths, "launch_strongest_paths", None, None, None, None, None, None)
        shape = tuple(self.shape)
        sp = StrongestPaths(
            power=np.empty((k,) + shape, np.float32),
            length=np.empty((k,) + shape, np.float32),
            cand=np.empty((k,) + shape + (L.D2D_MAX_ORDER,), np.int32),
            order=np.empty((k,) + shape, np.int32),
            total=np.empty(shape, np.float32),
            count=np.empty(shape, np.int32),
        )
        L.check(self._lib.d2d_get_strongest_paths(self._ctx, *(a.ctypes.data_as(C.c_void_p) for a in sp)))
        return sp

    def coherent_field(self, params: L.Params, fixed, inv_wavelength: float, amplitude="sqrt") -> "CoherentField":
        """The coherent sum of every cell of the resident grid at one wavelength: the fused sweep's contributions ``valid * fun``
        as complex amplitudes with the phase of their path length, ``sum a * e^(-j 2 pi r * inv_wavelength)`` -- one launch of the
        coherent-field build of the culled sweep (include/d2d.h: d2d_coherent_field_launch holds the definition; ImagePath, hard or
        hard_sigmoid validity, every fused function).  ``inv_wavelength`` is ``1 / lambda`` in turns per unit length, finite and
        ``>= 0``; ``amplitude`` is ``"sqrt"`` (the fused function is a power: its amplitude is the square root, its sign a pi flip)
        or ``"linear"`` (the fused function is the amplitude), or the library's constant.  ``params.grid_role`` says which end of
        the paths the cells are, ``fixed`` is the other end.  The resident value map, the records of :meth:`valid_paths`, the
        profile and the strongest paths are not touched.

        Returns a :class:`CoherentField`: ``re``, ``im`` and ``total`` (the fused map, bit for bit), fp32 ``[m, n]`` each.
        :func:`differt2d_amd.utils.field_power` and :func:`differt2d_amd.utils.fading_gain` turn it into a power and into the
        gain of the coherent sum over the incoherent one."""
        self.launch_coherent_field(params, fixed, inv_wavelength, amplitude)
        return self.get_coherent_field()

    def launch_coherent_field(self, params: L.Params, fixed, inv_wavelength: float, amplitude="sqrt"):
        """The launch of :meth:`coherent_field` alone (asynchronous, like :meth:`launch`)."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        self._field = False
        amplitude = _amplitude_id("coherent_field", amplitude)
        L.check(self._lib.d2d_coherent_field_launch(self._ctx, C.byref(params), fixed, float(inv_wavelength), amplitude))
        self._field = True

    def get_coherent_field(self) -> "CoherentField":
        """Synchronises and returns the result of the last :meth:`launch_coherent_field`."""
        if not self._field:
            _no_result(self._ctx, self._lib.d2d_get_coherent_field, "launch_coherent_field", None, None, None)
        shape = tuple(self.shape)
        cf = CoherentField(re=np.empty(shape, np.float32), im=np.empty(shape, np.float32), total=np.empty(shape, np.float32))
        L.check(self._lib.d2d_get_coherent_field(self._ctx, *(a.ctypes.data_as(C.c_void_p) for a in cf)))
        return cf

    def frequency_response(self, params: L.Params, fixed, inv_wavelengths, amplitude="sqrt") -> "FrequencyResponse":
        """The channel frequency response of every cell of the resident grid: the coherent sum of :meth:`coherent_field` at every
        entry of ``inv_wavelengths`` (``1 / lambda_j`` in turns per unit length: fp32, finite and ``>= 0``, 1 to
        ``D2D_FREQ_MAX`` = 1024 entries) from ONE preparation of the culled sweep and one kernel pass per 8 entries, where a
        :meth:`coherent_field` call per entry repeats the whole sweep (include/d2d.h: d2d_frequency_response_launch holds the
        definition).  Plane ``j`` equals ``coherent_field(params, fixed, inv_wavelengths[j], amplitude)`` bit for bit, whatever
        else the list holds.  ``amplitude``, ``params`` and ``fixed`` as for :meth:`coherent_field`.  The resident value map, the
        records of :meth:`valid_paths`, the profile, the strongest paths and the coherent field are not touched.

        Returns a :class:`FrequencyResponse`: ``re`` and ``im``, fp32 ``[nf, m, n]``, and ``total`` (the fused map, bit for bit),
        fp32 ``[m, n]``.  :func:`differt2d_amd.utils.frequency_response`, :func:`differt2d_amd.utils.wideband_power` and
        :func:`differt2d_amd.utils.impulse_response` turn it into complex ``H``, the frequency-averaged power and the taps of the
        coherent impulse response."""
        self.launch_frequency_response(params, fixed, inv_wavelengths, amplitude)
        return self.get_frequency_response()

    def launch_frequency_response(self, params: L.Params, fixed, inv_wavelengths, amplitude="sqrt"):
        """The launch of :meth:`frequency_response` alone (asynchronous, like :meth:`launch`; the list is copied by the call)."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        inv = np.ascontiguousarray(inv_wavelengths, dtype=np.float32).reshape(-1)
        self._freq_nf = 0
        amplitude = _amplitude_id("frequency_response", amplitude)
        keep = _keep_pointer(inv, 1)
        L.check(self._lib.d2d_frequency_response_launch(self._ctx, C.byref(params), fixed, keep.ctypes.data_as(C.c_void_p), int(inv.size),
                                                        amplitude))
        self._freq_nf = int(inv.size)

    def _read_frequency_response(self, getter, nf: int) -> "FrequencyResponse":
        """``nf`` planes ``re`` / ``im`` and ``total`` of the resident grid's shape, filled by ``getter``."""
        shape = tuple(self.shape)
        planes = (nf,) + shape
        fr = FrequencyResponse(re=np.empty(planes, np.float32), im=np.empty(planes, np.float32), total=np.empty(shape, np.float32))
        L.check(getter(self._ctx, *(a.ctypes.data_as(C.c_void_p) for a in fr)))
        return fr

    def get_frequency_response(self) -> "FrequencyResponse":
        """Synchronises and returns the result of the last :meth:`launch_frequency_response`."""
        if not self._freq_nf:
            _no_result(self._ctx, self._lib.d2d_get_frequency_response, "launch_frequency_response", None, None, None)
        return self._read_frequency_response(self._lib.d2d_get_frequency_response, self._freq_nf)

    def material_response(self, params: L.Params, fixed, inv_wavelengths, permittivity, polarization="te",
                          amplitude="sqrt") -> "FrequencyResponse":
        """:meth:`frequency_response` with Fresnel reflection per wall: every contribution is multiplied by the product of the
        complex reflection coefficients of the walls it bounces off, each a function of the angle of incidence, of
        ``polarization`` (``"te"``: E perpendicular to the plane of incidence -- for vertical antennas over a 2-D floor plan E
        out of the plane, the default; ``"tm"``: E in the plane of incidence) and of the wall's complex relative permittivity
        (include/d2d.h: d2d_material_response_launch holds the definition, differt2d_amd/csrc/d2d_fresnel.hpp the coefficient;
        :func:`differt2d_amd.utils.fresnel_coefficient` is the same formula in complex128).  ONE preparation of the culled
        sweep, one kernel pass per 8 wavelengths.

        ``permittivity``: complex ``[N]``, one value per object of the scene for the whole band, or ``[nf, N]``, a row per entry
        of ``inv_wavelengths``.  The time convention is the library's, ``e^(-j 2 pi r / lambda)``: a lossy medium is
        ``eps' - 1j * eps''``, so the imaginary part is ``<= 0`` (:func:`differt2d_amd.utils.complex_permittivity`).  Pass
        ``params`` whose path function holds no reflection loss of its own (``received_power`` with ``r_coef = 1``, or
        ``one``), so that walls are not counted twice.  ``amplitude``, ``params`` and ``fixed`` as for :meth:`coherent_field`.
        No other product's result is touched.  Values only, one GPU.

        Returns a :class:`FrequencyResponse`: ``re`` and ``im``, fp32 ``[nf, m, n]``, and ``total`` (the fused map, bit for bit),
        fp32 ``[m, n]`` -- :func:`differt2d_amd.utils.frequency_response`, :func:`~differt2d_amd.utils.wideband_power`,
        :func:`~differt2d_amd.utils.impulse_response` and :func:`~differt2d_amd.utils.field_misfit` apply unchanged."""
        self.launch_material_response(params, fixed, inv_wavelengths, permittivity, polarization, amplitude)
        return self.get_material_response()

    def launch_material_response(self, params: L.Params, fixed, inv_wavelengths, permittivity, polarization="te", amplitude="sqrt"):
        """The launch of :meth:`material_response` alone (asynchronous, like :meth:`launch`; the lists are copied by the call).  A
        refused launch leaves the previous result readable."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        inv = np.ascontiguousarray(inv_wavelengths, dtype=np.float32).reshape(-1)
        eps = _permittivity_table("material_response", permittivity, int(inv.size))
        amplitude = _amplitude_id("material_response", amplitude)
        polarization = _polarization_id("material_response", polarization)
        keep, table = _keep_pointer(inv, 1), _keep_pointer(eps.view(np.float32), 2)
        L.check(self._lib.d2d_material_response_launch(self._ctx, C.byref(params), fixed, keep.ctypes.data_as(C.c_void_p), int(inv.size), amplitude,
                                                       polarization, table.ctypes.data_as(C.c_void_p), int(eps.shape[1])))
        self._mat_nf = int(inv.size)

    def get_material_response(self) -> "FrequencyResponse":
        """Synchronises and returns the result of the last :meth:`launch_material_response` that was accepted."""
        if not self._mat_nf:
            _no_result(self._ctx, self._lib.d2d_get_material_response, "launch_material_response", None, None, None)
        return self._read_frequency_response(self._lib.d2d_get_material_response, self._mat_nf)

    def material_eps_vjp(self, params: L.Params, fixed, inv_wavelengths, permittivity, re_bar, im_bar, polarization="te",
                         amplitude="sqrt") -> np.ndarray:
        """The reverse-mode product of :meth:`material_response` with respect to the walls' permittivities: ``eps_bar[f, w] =
        dL/dRe eps[f, w] + 1j * dL/dIm eps[f, w]`` for ``dL = sum (re_bar * d re + im_bar * d im)``, complex128 ``[nf, N]``, from
        ONE preparation of the culled sweep and, per 8 wavelengths, one kernel pass and one fixed-order fp64 reduction
        (include/d2d.h: d2d_material_eps_vjp_launch holds the definition, differt2d_amd/csrc/d2d_fresnel_grad.hpp the derivative
        of the coefficient).  ``eps - rate * eps_bar`` is a step of gradient descent.

        ``params``, ``fixed``, ``inv_wavelengths``, ``permittivity``, ``polarization`` and ``amplitude`` are
        :meth:`material_response`'s, refused alike; a ``permittivity`` of shape ``[N]`` stands for equal rows and the result still
        has a row per wavelength (sum them for the gradient of the one value).  ``re_bar`` and ``im_bar`` are the cotangents of
        the planes, ``[nf, m, n]`` (taken as fp32, copied by the call; non-finite values propagate):
        :func:`differt2d_amd.utils.field_misfit` gives them for a least-squares fit.  Walls that no contributing path touches
        get exactly ``+0.0``.  The same bits run to run.  A refused launch leaves the previous result readable; no other
        product's result is touched."""
        self.launch_material_eps_vjp(params, fixed, inv_wavelengths, permittivity, re_bar, im_bar, polarization, amplitude)
        return self.get_material_eps_vjp()

    def launch_material_eps_vjp(self, params: L.Params, fixed, inv_wavelengths, permittivity, re_bar, im_bar, polarization="te",
                                amplitude="sqrt"):
        """The launch of :meth:`material_eps_vjp` alone (the lists and the cotangents are copied by the call; the kernels are
        asynchronous, like :meth:`launch`)."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        inv = np.ascontiguousarray(inv_wavelengths, dtype=np.float32).reshape(-1)
        eps = _permittivity_table("material_eps_vjp", permittivity, int(inv.size))
        amplitude = _amplitude_id("material_eps_vjp", amplitude)
        polarization = _polarization_id("material_eps_vjp", polarization)
        keep, table = _keep_pointer(inv, 1), _keep_pointer(eps.view(np.float32), 2)
        rb, ib = _cotangent_planes("material_eps_vjp", re_bar, im_bar, int(inv.size), self.shape, keep)
        L.check(self._lib.d2d_material_eps_vjp_launch(self._ctx, C.byref(params), fixed, keep.ctypes.data_as(C.c_void_p), int(inv.size), amplitude,
                                                      polarization, table.ctypes.data_as(C.c_void_p), int(eps.shape[1]),
                                                      rb.ctypes.data_as(C.c_void_p), ib.ctypes.data_as(C.c_void_p)))
        self._eps_vjp_nf = int(inv.size)

    def get_material_eps_vjp(self) -> np.ndarray:
        """Synchronises and returns the result of the last :meth:`launch_material_eps_vjp` that was accepted: complex128
        ``[nf, N]``."""
        if not self._eps_vjp_nf:
            _no_result(self._ctx, self._lib.d2d_get_material_eps_vjp, "launch_material_eps_vjp", None)
        n = self._eps_vjp_nf * self.n_objects
        out = np.zeros(max(n, 1), np.complex128)  # (re, im) pairs of float64: the library's layout
        L.check(self._lib.d2d_get_material_eps_vjp(self._ctx, out.ctypes.data_as(C.c_void_p)))
        return out[:n].reshape(self._eps_vjp_nf, self.n_objects)

    def field_coefs_vjp(self, params: L.Params, fixed, inv_wavelengths, re_bar, im_bar, amplitude="sqrt") -> np.ndarray:
        """The reverse-mode product of :meth:`frequency_response` with respect to the per-object reflection coefficients:
        ``coef_bar[w] = sum_j sum_cells (re_bar * d re / d coef[w] + im_bar * d im / d coef[w])``, float64 ``[N]``, from ONE
        preparation of the culled sweep and one kernel pass per 8 wavelengths, as the forward product (include/d2d.h:
        d2d_field_coefs_vjp_launch holds the definition).  ``params.fun`` must be ``received_power_per_object`` with the
        coefficients of :meth:`set_reflection_coefs`; ``inv_wavelengths`` and ``amplitude`` as for :meth:`frequency_response`;
        ``re_bar`` and ``im_bar`` are the cotangents of its planes, ``[nf, m, n]`` (taken as fp32, copied by the call; non-finite
        values propagate).  A coefficient of zero has a gradient with ``"linear"``; with ``"sqrt"`` a candidate whose coefficients
        multiply to zero adds no term.  Walls that no contributing path touches get exactly ``+0.0``.  A refused launch leaves the
        previous result readable.  The resident value map, the scene VJP of :meth:`launch_vg` and the other products' results are
        not touched.  :func:`differt2d_amd.utils.field_misfit` gives the loss and the cotangents of a least-squares fit."""
        self.launch_field_coefs_vjp(params, fixed, inv_wavelengths, re_bar, im_bar, amplitude)
        return self.get_field_coefs_vjp()

    def launch_field_coefs_vjp(self, params: L.Params, fixed, inv_wavelengths, re_bar, im_bar, amplitude="sqrt"):
        """The launch of :meth:`field_coefs_vjp` alone (the list and the cotangents are copied by the call; the kernels are
        asynchronous, like :meth:`launch`)."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        inv = np.ascontiguousarray(inv_wavelengths, dtype=np.float32).reshape(-1)
        amplitude = _amplitude_id("field_coefs_vjp", amplitude)
        keep = _keep_pointer(inv, 1)
        rb, ib = _cotangent_planes("field_coefs_vjp", re_bar, im_bar, int(inv.size), self.shape, keep)
        L.check(self._lib.d2d_field_coefs_vjp_launch(self._ctx, C.byref(params), fixed, keep.ctypes.data_as(C.c_void_p), int(inv.size),
                                                     amplitude, rb.ctypes.data_as(C.c_void_p), ib.ctypes.data_as(C.c_void_p)))

    def get_field_coefs_vjp(self) -> np.ndarray:
        """Synchronises and returns the result of the last :meth:`launch_field_coefs_vjp` that was accepted: float64 ``[N]``."""
        out = np.zeros(max(self.n_objects, 1), np.float64)
        L.check(self._lib.d2d_get_field_coefs_vjp(self._ctx, out.ctypes.data_as(C.c_void_p)))
        return out[: self.n_objects]

    def field_position_vjp(self, params: L.Params, fixed, inv_wavelengths, re_bar, im_bar, amplitude="sqrt") -> "PositionGradient":
        """The reverse-mode product of :meth:`frequency_response` with respect to positions: for a loss ``L`` with
        ``dL = sum (re_bar * d re + im_bar * d im)``, the gradient with respect to the position of every cell (the receiver of that
        cell on an RX grid, the transmitter on a TX grid) and with respect to the fixed end point, from ONE preparation of the
        culled sweep and one kernel pass per 8 wavelengths (include/d2d.h: d2d_field_position_vjp_launch holds the definition).
        Hard validity only: a position then enters through the path length alone, and the interaction points are stationary.
        ``params`` (any fused ``fun``), ``fixed``, ``inv_wavelengths`` and ``amplitude`` as for :meth:`frequency_response`;
        ``re_bar`` and ``im_bar`` are the cotangents of its planes, ``[nf, m, n]`` (taken as fp32, copied by the call; non-finite
        values propagate into their cell and ``fixed_bar``).  A refused launch leaves the previous result readable.  The resident
        value and gradient maps, the scene VJP of :meth:`launch_vg` and the other products' results are not touched.

        Returns a :class:`PositionGradient`: ``cell_bar`` and ``fixed_terms``, fp32 ``[m, n, 2]`` (indexed like
        :meth:`get_grad_rx`; views of the library's ``[2][m][n]`` planes), defined bit for bit, and ``fixed_bar``, float64 ``[2]``, the
        fixed-order sum of ``fixed_terms`` over the cells.  :func:`differt2d_amd.utils.field_misfit` gives the cotangents of a
        least-squares fit (localisation), :func:`differt2d_amd.utils.wideband_power_cotangent` those of the coherent wideband
        coverage (placement)."""
        self.launch_field_position_vjp(params, fixed, inv_wavelengths, re_bar, im_bar, amplitude)
        return self.get_field_position_vjp()

    def launch_field_position_vjp(self, params: L.Params, fixed, inv_wavelengths, re_bar, im_bar, amplitude="sqrt"):
        """The launch of :meth:`field_position_vjp` alone (the list and the cotangents are copied by the call; the kernels are
        asynchronous, like :meth:`launch`)."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        inv = np.ascontiguousarray(inv_wavelengths, dtype=np.float32).reshape(-1)
        amplitude = _amplitude_id("field_position_vjp", amplitude)
        keep = _keep_pointer(inv, 1)
        rb, ib = _cotangent_planes("field_position_vjp", re_bar, im_bar, int(inv.size), self.shape, keep)
        L.check(self._lib.d2d_field_position_vjp_launch(self._ctx, C.byref(params), fixed, keep.ctypes.data_as(C.c_void_p), int(inv.size),
                                                        amplitude, rb.ctypes.data_as(C.c_void_p), ib.ctypes.data_as(C.c_void_p)))

    def get_field_position_vjp(self) -> "PositionGradient":
        """Synchronises and returns the result of the last :meth:`launch_field_position_vjp` that was accepted."""
        if not self.shape:
            _no_result(self._ctx, self._lib.d2d_get_field_position_vjp, "launch_field_position_vjp", None, None, None)
        planes = (2,) + tuple(self.shape)
        cell, terms, bar = np.empty(planes, np.float32), np.empty(planes, np.float32), np.empty(2, np.float64)
        L.check(self._lib.d2d_get_field_position_vjp(self._ctx, *(a.ctypes.data_as(C.c_void_p) for a in (cell, terms, bar))))
        # (views of the library's [2][m][n] planes: no copy on the host)
        return PositionGradient(cell_bar=np.moveaxis(cell, 0, -1), fixed_terms=np.moveaxis(terms, 0, -1), fixed_bar=bar)

    def field_walls_vjp(self, params: L.Params, fixed, inv_wavelengths, re_bar, im_bar, amplitude="sqrt") -> "WallGradient":
        """The reverse-mode product of :meth:`frequency_response` with respect to the end points of every wall: for a loss ``L``
        with ``dL = sum (re_bar * d re + im_bar * d im)``, the gradient with respect to the two end points of every object of
        the resident scene, from ONE preparation of the culled sweep and one kernel pass per 8 wavelengths (include/d2d.h:
        d2d_field_walls_vjp_launch holds the definition).  Hard validity only: a wall then enters through the path length alone,
        and the interaction points are stationary.  The arguments are those of :meth:`field_position_vjp`.  A refused launch
        leaves the previous result readable.  The resident value and gradient maps, the scene VJP of :meth:`launch_vg` and the
        other products' results are not touched.

        Returns a :class:`WallGradient`: ``normal_bar``, float64 ``[N, 2]``, the sensitivity of ``L`` to moving end point ``A``
        or ``B`` of a wall along the wall's unit normal, and ``walls_bar``, float64 ``[N, 2, 2]`` (the layout of
        :meth:`get_scene_vjp`'s ``objects_bar``), ``normal_bar`` times the wall's fp32 unit normal.  Fixed-order sums: the same
        bits run to run, within a derived bound of a float64 evaluation.  :func:`differt2d_amd.utils.field_misfit` gives the
        cotangents of a least-squares fit to a measured channel (wall localisation)."""
        self.launch_field_walls_vjp(params, fixed, inv_wavelengths, re_bar, im_bar, amplitude)
        return self.get_field_walls_vjp()

    def launch_field_walls_vjp(self, params: L.Params, fixed, inv_wavelengths, re_bar, im_bar, amplitude="sqrt"):
        """The launch of :meth:`field_walls_vjp` alone (the list and the cotangents are copied by the call; the kernels are
        asynchronous, like :meth:`launch`)."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        inv = np.ascontiguousarray(inv_wavelengths, dtype=np.float32).reshape(-1)
        amplitude = _amplitude_id("field_walls_vjp", amplitude)
        keep = _keep_pointer(inv, 1)
        rb, ib = _cotangent_planes("field_walls_vjp", re_bar, im_bar, int(inv.size), self.shape, keep)
        L.check(self._lib.d2d_field_walls_vjp_launch(self._ctx, C.byref(params), fixed, keep.ctypes.data_as(C.c_void_p), int(inv.size),
                                                     amplitude, rb.ctypes.data_as(C.c_void_p), ib.ctypes.data_as(C.c_void_p)))

    def get_field_walls_vjp(self) -> "WallGradient":
        """Synchronises and returns the result of the last :meth:`launch_field_walls_vjp` that was accepted."""
        n = self.n_objects
        walls, normal = np.zeros((max(n, 1), 2, 2), np.float64), np.zeros((max(n, 1), 2), np.float64)
        L.check(self._lib.d2d_get_field_walls_vjp(self._ctx, walls.ctypes.data_as(C.c_void_p), normal.ctypes.data_as(C.c_void_p)))
        return WallGradient(walls_bar=walls[:n], normal_bar=normal[:n])

    def selftest_wallgrad(self, G, qx, qy, sx, sy, ox, oy, nx, ny, tx, ty, sq):
        """``(qx, qy, Wa, Wb, ok)`` of d2d_wallgrad.hpp's ``wallgrad_bounce`` on the device (include/d2d.h: d2d_selftest_wallgrad):
        twelve arrays of one size."""
        cols = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in (G, qx, qy, sx, sy, ox, oy, nx, ny, tx, ty, sq)]
        if len({c.size for c in cols}) != 1:
            raise ValueError("selftest_wallgrad: arrays of one size")
        ptrs = (C.c_void_p * 12)(*(c.ctypes.data for c in cols))
        outs = [np.empty_like(cols[0]) for _ in range(5)]
        L.check(self._lib.d2d_selftest_wallgrad(self._ctx, ptrs, cols[0].size, *outs))
        return tuple(outs)

    def selftest_posgrad(self, fun_id: int, amplitude, t, r, h2, inv, rb, ib):
        """``(a, rho, kr, g, G)`` of d2d_posgrad.hpp on the device (include/d2d.h: d2d_selftest_posgrad): ``inv``, ``rb`` and ``ib`` are
        ``[2, n]``, the two wavelengths of the fold; the other inputs ``[n]``."""
        t, r, h2 = (np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in (t, r, h2))
        pairs = [np.ascontiguousarray(x, dtype=np.float32).reshape(2, t.size) for x in (inv, rb, ib)]
        if not (t.size == r.size == h2.size):
            raise ValueError("selftest_posgrad: arrays of one size")
        outs = [np.empty_like(t) for _ in range(5)]
        L.check(self._lib.d2d_selftest_posgrad(self._ctx, int(fun_id), _amplitude_id("selftest_posgrad", amplitude), t, r, h2,
                                               *(np.ascontiguousarray(p[k]) for p in pairs for k in (0, 1)), t.size, *outs))
        return tuple(outs)

    def power_angle(self, params: L.Params, fixed, end, origin_turns: float, nbins: int) -> "PowerAngleProfile":
        """The power-angle profile of every cell of the resident grid: the fused sweep's contributions ``valid * fun`` binned by
        the direction in which their path leaves the transmitter (``end="tx"``, departure) or by the direction from the receiver
        towards the last interaction point (``end="rx"``, arrival) -- one launch of the power-angle build of the culled sweep
        (include/d2d.h: d2d_power_angle_launch holds the definition, the angle's arithmetic included; ImagePath, hard or
        hard_sigmoid validity, every fused function).  ``end`` may also be the library's constant.  ``nbins`` equal bins cover the
        full turn counter-clockwise from ``origin_turns`` (fp32, in turns, ``0 <= origin_turns < 1``, measured from +x);
        ``1 <= nbins <= 4096``.  ``params.grid_role`` says which end of the paths the cells are, ``fixed`` is the other end:
        ``"tx"`` over an RX grid and ``"rx"`` over a TX grid bin at the fixed end point, the other two at the cell.  A refused launch
        leaves the previous result readable.  The resident value map, the records of :meth:`valid_paths`, the delay profile, the
        strongest paths, the coherent field and the frequency response are not touched.

        Returns a :class:`PowerAngleProfile`: ``bins`` fp32 ``[nbins, m, n]`` and ``total`` (the fused map, bit for bit), fp32
        ``[m, n]``.  :func:`differt2d_amd.utils.angular_statistics` and :func:`differt2d_amd.utils.pattern_power` turn it into the
        mean direction and angular spread and into the power a directional antenna receives."""
        self.launch_power_angle(params, fixed, end, origin_turns, nbins)
        return self.get_power_angle()

    def launch_power_angle(self, params: L.Params, fixed, end, origin_turns: float, nbins: int):
        """The launch of :meth:`power_angle` alone (asynchronous, like :meth:`launch`)."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        if isinstance(end, str):
            if end not in ANGLE_ENDS:
                raise L.D2DError(-1, f"power_angle: end must be one of {sorted(ANGLE_ENDS)}, got {end!r}")
            end = ANGLE_ENDS[end]
        L.check(self._lib.d2d_power_angle_launch(self._ctx, C.byref(params), fixed, int(end), float(origin_turns), int(nbins)))
        self._angle_nbins = int(nbins)

    def get_power_angle(self) -> "PowerAngleProfile":
        """Synchronises and returns the result of the last :meth:`launch_power_angle` that was accepted."""
        if not self._angle_nbins:
            _no_result(self._ctx, self._lib.d2d_get_power_angle, "launch_power_angle", None, None)
        shape = tuple(self.shape)
        pa = PowerAngleProfile(bins=np.empty((self._angle_nbins,) + shape, np.float32), total=np.empty(shape, np.float32))
        L.check(self._lib.d2d_get_power_angle(self._ctx, *(a.ctypes.data_as(C.c_void_p) for a in pa)))
        return pa

    def array_response(self, params: L.Params, fixed, inv_wavelength: float, tx_elements, rx_elements, amplitude="sqrt") -> "ArrayResponse":
        """The channel matrix of every cell of the resident grid between a transmit array and a receive array: the coherent sum of
        :meth:`coherent_field` for every pair of a transmit element ``j`` and a receive element ``i``, each contribution's phase
        steered by the plane-wave model, ``(r - e_tx[j] . u_tx - e_rx[i] . u_rx) * inv_wavelength`` turns with the unit directions
        of departure and arrival -- one launch of the array-response build of the culled sweep (include/d2d.h:
        d2d_array_response_launch holds the definition; ImagePath, hard or hard_sigmoid validity, every fused function).
        ``tx_elements`` ``[nt, 2]`` and ``rx_elements`` ``[nr, 2]`` are element offsets ``(ex, ey)`` in length units from the
        terminal's position, finite, 1 to ``D2D_ARRAY_MAX`` = 8 of each (:func:`differt2d_amd.utils.ula` makes a uniform linear
        array); the transmit array sits at the transmitter and the receive array at the receiver in both grid roles.
        ``inv_wavelength``, ``amplitude``, ``params`` and ``fixed`` as for :meth:`coherent_field`.  A pair of zero offsets equals
        :meth:`coherent_field` bit for bit wherever every path has a direction at both ends.  A refused launch leaves the previous
        result readable.  Every other product of the context is left untouched.

        Returns an :class:`ArrayResponse`: ``re`` and ``im``, fp32 ``[nr, nt, m, n]``, and ``total`` (the fused map, bit for bit),
        fp32 ``[m, n]``.  :func:`differt2d_amd.utils.channel_matrix`, :func:`differt2d_amd.utils.beamformed_power`,
        :func:`differt2d_amd.utils.singular_values` and :func:`differt2d_amd.utils.mimo_capacity` turn it into complex ``H``, the
        power behind two beamformers, the singular values and the capacity of every cell."""
        self.launch_array_response(params, fixed, inv_wavelength, tx_elements, rx_elements, amplitude)
        return self.get_array_response()

    def launch_array_response(self, params: L.Params, fixed, inv_wavelength: float, tx_elements, rx_elements, amplitude="sqrt"):
        """The launch of :meth:`array_response` alone (asynchronous, like :meth:`launch`; the lists are copied by the call)."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        etx = np.ascontiguousarray(tx_elements, dtype=np.float32).reshape(-1, 2)
        erx = np.ascontiguousarray(rx_elements, dtype=np.float32).reshape(-1, 2)
        amplitude = _amplitude_id("array_response", amplitude)
        ktx, krx = _keep_pointer(etx, 1, 2), _keep_pointer(erx, 1, 2)
        L.check(self._lib.d2d_array_response_launch(self._ctx, C.byref(params), fixed, float(inv_wavelength), amplitude, int(etx.shape[0]),
                                                    ktx, int(erx.shape[0]), krx))
        self._array_shape = (int(erx.shape[0]), int(etx.shape[0]))

    def get_array_response(self) -> "ArrayResponse":
        """Synchronises and returns the result of the last :meth:`launch_array_response` that was accepted."""
        if self._array_shape is None:
            _no_result(self._ctx, self._lib.d2d_get_array_response, "launch_array_response", None, None, None)
        shape = tuple(self.shape)
        planes = self._array_shape + shape
        ar = ArrayResponse(re=np.empty(planes, np.float32), im=np.empty(planes, np.float32), total=np.empty(shape, np.float32))
        L.check(self._lib.d2d_get_array_response(self._ctx, *(a.ctypes.data_as(C.c_void_p) for a in ar)))
        return ar

    def array_frequency_response(self, params: L.Params, fixed, inv_wavelengths, tx_elements, rx_elements,
                                 amplitude="sqrt") -> "ArrayFrequencyResponse":
        """The channel matrices of every cell of the resident grid at many wavelengths: :meth:`array_response` at every entry of
        ``inv_wavelengths`` (``1 / lambda_f`` in turns per unit length: fp32, finite and ``>= 0``, 1 to ``D2D_FREQ_MAX`` = 1024
        entries) from ONE check, preparation and zeroing and one kernel pass per chunk of entries, where an :meth:`array_response`
        call per entry repeats them and the whole culled sweep (include/d2d.h: d2d_array_frequency_response_launch holds the
        definition).  Plane block ``f`` equals ``array_response(params, fixed, inv_wavelengths[f], tx_elements, rx_elements,
        amplitude)`` bit for bit, whatever else the lists hold; a pair of zero offsets equals :meth:`frequency_response` bit for
        bit wherever every path has a direction at both ends.  ``tx_elements``, ``rx_elements``, ``amplitude``, ``params`` and
        ``fixed`` as for :meth:`array_response`.  A refused launch leaves the previous result readable.  Every other product of
        the context is left untouched.

        Returns an :class:`ArrayFrequencyResponse`: ``re`` and ``im``, fp32 ``[nf, nr, nt, m, n]``, and ``total`` (the fused map,
        bit for bit), fp32 ``[m, n]``.  :func:`differt2d_amd.utils.channel_tensor`, :func:`differt2d_amd.utils.array_response_at`
        and :func:`differt2d_amd.utils.wideband_capacity` turn it into complex ``H``, the :class:`ArrayResponse` of one
        wavelength and the capacity averaged over the band.  The result takes ``8 * nf * nr * nt`` bytes per cell:
        :meth:`get_array_frequency_response` reads a range of wavelengths where the whole does not fit the host."""
        self.launch_array_frequency_response(params, fixed, inv_wavelengths, tx_elements, rx_elements, amplitude)
        return self.get_array_frequency_response()

    def launch_array_frequency_response(self, params: L.Params, fixed, inv_wavelengths, tx_elements, rx_elements, amplitude="sqrt"):
        """The launch of :meth:`array_frequency_response` alone (asynchronous, like :meth:`launch`; the lists are copied by the call)."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        inv = np.ascontiguousarray(inv_wavelengths, dtype=np.float32).reshape(-1)
        etx = np.ascontiguousarray(tx_elements, dtype=np.float32).reshape(-1, 2)
        erx = np.ascontiguousarray(rx_elements, dtype=np.float32).reshape(-1, 2)
        amplitude = _amplitude_id("array_frequency_response", amplitude)
        kinv, ktx, krx = _keep_pointer(inv, 1), _keep_pointer(etx, 1, 2), _keep_pointer(erx, 1, 2)
        L.check(self._lib.d2d_array_frequency_response_launch(self._ctx, C.byref(params), fixed, kinv, int(inv.size), amplitude,
                                                              int(etx.shape[0]), ktx, int(erx.shape[0]), krx))
        self._wide_shape = (int(inv.size), int(erx.shape[0]), int(etx.shape[0]))

    def get_array_frequency_response(self, first=0, count=None, with_total=True) -> "ArrayFrequencyResponse":
        """Synchronises and returns wavelengths ``first .. first + count - 1`` (``count=None``: all from ``first`` on) of the result
        of the last :meth:`launch_array_frequency_response` that was accepted: ``re`` and ``im`` are ``[count, nr, nt, m, n]``.
        ``with_total=False`` leaves ``total`` out (``None``).  A range outside the result is refused by the library."""
        if self._wide_shape is None:
            _no_result(self._ctx, self._lib.d2d_get_array_frequency_response, "launch_array_frequency_response", 0, 1, None, None, None)
        nf, nr, nt = self._wide_shape
        first = int(first)
        count = nf - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > nf:  # (the library says why: nothing is copied)
            L.check(self._lib.d2d_get_array_frequency_response(self._ctx, first, count, None, None, None))
            raise L.D2DError(-1, f"get_array_frequency_response: first={first}, count={count} are no range of {nf} wavelengths")
        shape = tuple(self.shape)
        planes = (count, nr, nt) + shape
        afr = ArrayFrequencyResponse(re=np.empty(planes, np.float32), im=np.empty(planes, np.float32),
                                     total=np.empty(shape, np.float32) if with_total else None)
        L.check(self._lib.d2d_get_array_frequency_response(self._ctx, first, count,
                                                           *(None if a is None else a.ctypes.data_as(C.c_void_p) for a in afr)))
        return afr

    def beam_response(self, params: L.Params, fixed, inv_wavelengths, tx_elements, rx_elements, tx_weights, rx_weights,
                      amplitude="sqrt") -> "BeamResponse":
        """What comes out behind beamformers at both ends, ``y[f, br, bt] = w_rx[br]^H H[f] w_tx[bt]`` for every cell of the resident
        grid, every entry of ``inv_wavelengths`` and every pair of a receive beam and a transmit beam -- the channel tensor ``H`` of
        :meth:`array_frequency_response` contracted with two codebooks inside the sweep, without ``H`` ever being formed, stored or
        downloaded (include/d2d.h: d2d_beam_response_launch holds the definition; ImagePath, hard or hard_sigmoid validity, every
        fused function).  Under the plane-wave model every path's contribution to ``H`` has rank one, so per contribution and
        wavelength ``nt + nr + 1`` phasors are formed instead of ``nr * nt``, and ``nbr * nbt`` planes are written instead of
        ``nr * nt``.  ``tx_weights`` is complex ``[nbt, nt]`` (or ``[nt]`` for one beam) and ``rx_weights`` complex ``[nbr, nr]``
        (or ``[nr]``), 1 to ``D2D_BEAM_MAX`` = 8 beams each, every component finite; they are passed as complex64.  The receive
        weights are conjugated, the convention of :func:`differt2d_amd.utils.beamformed_power`;
        :func:`differt2d_amd.utils.steering_weights` makes matched beams.  ``inv_wavelengths``, ``tx_elements``, ``rx_elements``,
        ``amplitude``, ``params`` and ``fixed`` as for :meth:`array_frequency_response`.  Plane ``(f, br, bt)`` depends only on
        ``inv_wavelengths[f]``, ``rx_weights[br]``, ``tx_weights[bt]`` and the element lists: a larger codebook is several calls.
        A refused launch leaves the previous result readable.  Every other product of the context is left untouched.

        Returns a :class:`BeamResponse`: ``re`` and ``im``, fp32 ``[nf, nbr, nbt, m, n]``, and ``total`` (the fused map, bit for
        bit), fp32 ``[m, n]``.  :func:`differt2d_amd.utils.beam_response`, :func:`differt2d_amd.utils.beam_power` and
        :func:`differt2d_amd.utils.best_beam` turn it into complex ``y``, the power of every pair and the best pair of every
        cell.  The result takes ``8 * nf * nbr * nbt`` bytes per cell: :meth:`get_beam_response` reads a range of wavelengths."""
        self.launch_beam_response(params, fixed, inv_wavelengths, tx_elements, rx_elements, tx_weights, rx_weights, amplitude)
        return self.get_beam_response()

    def launch_beam_response(self, params: L.Params, fixed, inv_wavelengths, tx_elements, rx_elements, tx_weights, rx_weights,
                             amplitude="sqrt"):
        """The launch of :meth:`beam_response` alone (asynchronous, like :meth:`launch`; the lists are copied by the call)."""
        fixed = np.ascontiguousarray(fixed, dtype=np.float32).reshape(2)
        inv = np.ascontiguousarray(inv_wavelengths, dtype=np.float32).reshape(-1)
        etx = np.ascontiguousarray(tx_elements, dtype=np.float32).reshape(-1, 2)
        erx = np.ascontiguousarray(rx_elements, dtype=np.float32).reshape(-1, 2)
        wtx = _beam_weights("tx_weights", tx_weights, int(etx.shape[0]))
        wrx = _beam_weights("rx_weights", rx_weights, int(erx.shape[0]))
        amplitude = _amplitude_id("beam_response", amplitude)
        kinv, ktx, krx = _keep_pointer(inv, 1), _keep_pointer(etx, 1, 2), _keep_pointer(erx, 1, 2)
        kwt, kwr = _keep_pointer(wtx.view(np.float32), 2), _keep_pointer(wrx.view(np.float32), 2)
        L.check(self._lib.d2d_beam_response_launch(self._ctx, C.byref(params), fixed, kinv, int(inv.size), amplitude, int(etx.shape[0]), ktx,
                                                   int(erx.shape[0]), krx, int(wtx.shape[0]), kwt, int(wrx.shape[0]), kwr))
        self._beam_shape = (int(inv.size), int(wrx.shape[0]), int(wtx.shape[0]))

    def get_beam_response(self, first=0, count=None, with_total=True) -> "BeamResponse":
        """Synchronises and returns wavelengths ``first .. first + count - 1`` (``count=None``: all from ``first`` on) of the result
        of the last :meth:`launch_beam_response` that was accepted: ``re`` and ``im`` are ``[count, nbr, nbt, m, n]``.
        ``with_total=False`` leaves ``total`` out (``None``).  A range outside the result is refused by the library."""
        if self._beam_shape is None:
            _no_result(self._ctx, self._lib.d2d_get_beam_response, "launch_beam_response", 0, 1, None, None, None)
        nf, nbr, nbt = self._beam_shape
        first = int(first)
        count = nf - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > nf:  # (the library says why: nothing is copied)
            L.check(self._lib.d2d_get_beam_response(self._ctx, first, count, None, None, None))
            raise L.D2DError(-1, f"get_beam_response: first={first}, count={count} are no range of {nf} wavelengths")
        shape = tuple(self.shape)
        planes = (count, nbr, nbt) + shape
        br = BeamResponse(re=np.empty(planes, np.float32), im=np.empty(planes, np.float32),
                          total=np.empty(shape, np.float32) if with_total else None)
        L.check(self._lib.d2d_get_beam_response(self._ctx, first, count, *(None if a is None else a.ctypes.data_as(C.c_void_p) for a in br)))
        return br

    # -- RCCL ---------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(L.D2D_COMM_ID_BYTES)
        L.check(L.load().d2d_comm_unique_id(C.cast(buf, C.c_void_p)))
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        if len(unique_id) != L.D2D_COMM_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        buf = C.create_string_buffer(unique_id, L.D2D_COMM_ID_BYTES)
        L.check(self._lib.d2d_comm_init(self._ctx, C.cast(buf, C.c_void_p), int(rank), int(world)))
        self.rank, self.world = int(rank), int(world)

    def comm_destroy(self):
        L.check(self._lib.d2d_comm_destroy(self._ctx))

    def comm_count(self) -> int:
        """Ranks of the communicator as RCCL reports them (ncclCommCount)."""
        n = C.c_int32(0)
        L.check(self._lib.d2d_comm_count(self._ctx, C.byref(n)))
        return int(n.value)

    def comm_allgather_map(self, grad: bool = False):
        L.check(self._lib.d2d_comm_allgather_map(self._ctx, 1 if grad else 0))

    def comm_gather_map(self, root: int = 0, grad: bool = False):
        """Gathers the resident map to ``root`` only (ncclSend / ncclRecv): only ``root`` may fetch it afterwards."""
        L.check(self._lib.d2d_comm_gather_map(self._ctx, 1 if grad else 0, int(root)))

    def comm_get_gathered(self, world: int, grad: bool = False) -> np.ndarray:
        shape = (world, *self.shape, 2) if grad else (world, *self.shape)
        out = np.empty(shape, np.float32)
        L.check(self._lib.d2d_comm_get_gathered(self._ctx, 1 if grad else 0, out.reshape(-1), out.size))
        return out

    def comm_allreduce_vjp(self):
        L.check(self._lib.d2d_comm_allreduce_vjp(self._ctx))

    def comm_allreduce_host(self, values, op: str = "sum") -> np.ndarray:
        """All-reduces a few host doubles over ranks through RCCL (synchronous)."""
        v = np.ascontiguousarray(np.atleast_1d(values), dtype=np.float64).copy()
        L.check(self._lib.d2d_comm_allreduce_host(self._ctx, v, v.size, {"sum": 0, "max": 1}[op]))
        return v

    def comm_barrier(self):
        """Stream-synchronising barrier over all ranks of the communicator."""
        self.comm_allreduce_host([1.0], "sum")

    # -- timing -----------------------------------------------------------------------
    def timer_begin(self):
        L.check(self._lib.d2d_timer_begin(self._ctx))

    def timer_end(self) -> float:
        ms = C.c_float(0.0)
        L.check(self._lib.d2d_timer_end(self._ctx, C.byref(ms)))
        return ms.value


_default_ctx = {}


def default_context(device: int = 0) -> Context:
    """Process-wide context per device (created on first use; raises without a GPU)."""
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
