"""The oracle of ``received_power_per_object``, built from ``oracle/ref.py``'s public pieces (the oracle itself is not edited):
loop over ``R.all_path_candidates``, fold the candidate's numerator from the left, hand ``R.accumulate_candidate`` a per-candidate
closure ``num / (h * h + r * r)`` over ``R.path_length``, add ``valid * f`` in candidate order.  ``tests/test_object_coefs_cpu.py``
pins the recipe itself; ``tests/test_gpu_object_coefs.py`` holds the kernels to it."""

import numpy as np

from oracle import ref as R

F = np.float32


class LibmBackend(R.NumpyBackend):
    """``R.NumpyBackend`` whose fp32 ``exp`` is the host C library's ``expf``.  NumPy's own fp32 ``exp`` is a SIMD routine that
    differs from libm's by an ulp in a third of the arguments, so a sigmoid map of the plain backend is not bit-comparable with
    anything; the repository's sigmoid oracle (oracle/d2d_oracle.c) and the device (d2d_kernels.hpp: expf_libm,
    tests/test_gpu_selftest.py) both evaluate libm's.  Here: the algorithm of glibc's expf restated in NumPy float64, one rounding
    per operation (scripts/check_expf_model.py checks the same restatement against libm; tests/test_object_coefs_cpu.py checks
    this one).  Every other operation is NumpyBackend's; only sigmoid validity calls ``exp``."""

    _N = 32
    _INV = float.fromhex("0x1.71547652b82fep+0") * 32
    _SHIFT = float.fromhex("0x1.8p+52")
    _C = (float.fromhex("0x1.c6af84b912394p-5") / 32 / 32 / 32, float.fromhex("0x1.ebfce50fac4f3p-3") / 32 / 32,
          float.fromhex("0x1.62e42ff0c52d6p-1") / 32)

    def __init__(self):
        import struct
        from decimal import Decimal, getcontext

        super().__init__(np.float32)
        getcontext().prec = 60
        tab = []
        for i in range(self._N):  # 2^(i/32), correctly rounded, minus i << 47 (glibc's __exp2f_data.tab)
            bits = struct.unpack("<Q", struct.pack("<d", float(Decimal(2) ** (Decimal(i) / Decimal(self._N)))))[0]
            tab.append((bits - (i << 47)) & 0xFFFFFFFFFFFFFFFF)
        self._tab = np.array(tab, np.uint64)

    def exp(self, x):
        x = np.asarray(x)
        if x.dtype != np.float32:
            return super().exp(x)
        c = self._C
        with np.errstate(all="ignore"):
            z = self._INV * x.astype(np.float64)
            kd = z + self._SHIFT
            ki = kd.view(np.uint64) if kd.ndim else np.atleast_1d(kd).view(np.uint64).reshape(())
            r = z - (kd - self._SHIFT)
            s = (self._tab[(ki & np.uint64(31)).astype(np.intp)] + (ki << np.uint64(47))).view(np.float64)
            y = (((c[0] * r + c[1]) * (r * r) + (c[2] * r + 1)) * s).astype(np.float32)
            if not (np.abs(x) < np.float32(87.0)).all():  # overflow, underflow, inf, NaN: expf's own branches
                y = np.where(x < np.float32(float.fromhex("-0x1.9d1d9ep6")), np.float32(2.0 ** -149), y)
                y = np.where(x > np.float32(float.fromhex("0x1.62e42ep6")), np.float32(np.inf), y)
                y = np.where(x < np.float32(float.fromhex("-0x1.9fe368p6")), np.float32(0.0), y)
                y = np.where(np.isnan(x), x, y).astype(np.float32)
        return y if x.ndim else np.float32(y.reshape(()))


def coef_map(walls, coef, fixed, Xg, Yg, min_order=0, max_order=1, height=0.1, approx=False, grid_role="rx", filter_nodes=None,
             xp=R.NUMPY, **kw):
    """``R.power_map`` with one reflection coefficient per wall.  ``coef``: fp32 array (NumPy backend) or a tensor (torch)."""
    objs = R.walls_to_objs(walls, xp)
    cands = R.all_path_candidates(len(objs), min_order, max_order, filter_nodes=filter_nodes)
    grid = R.vec(xp.asarray(Xg), xp.asarray(Yg), xp)
    fixed = xp.asarray(fixed)
    a, b = (fixed, grid) if grid_role == "rx" else (grid, fixed)
    h = xp.c(height)
    acc = xp.c(0.0) * R.X(grid)
    for cand in cands:
        num = xp.c(1.0)
        for o in cand:
            num = num * coef[int(o)]  # fp32, left fold, candidate order

        def fun(pts, xp=xp, num=num):
            r = R.path_length(pts, xp)
            return num / (h * h + r * r)

        valid, val, _, _ = R.accumulate_candidate(a, objs, cand, b, fun, None, "image", approx, xp, **kw)
        acc = acc + xp.to_float(valid) * val
    return acc


def coef_value_and_grads(walls, coef, fixed, Xg, Yg, cotangent=None, dtype="float32", **kw):
    """Torch autodiff of :func:`coef_map`: value, per-cell gradient w.r.t. the cell, and the VJP (``cotangent``, default ones) w.r.t.
    the fixed end point, the wall end points and the coefficients (a leaf tensor)."""
    import torch

    tb = R.TorchBackend(dtype)
    leaf = lambda x: tb.asarray(np.asarray(x)).clone().requires_grad_(True)
    w, c, t, gx, gy = leaf(walls), leaf(coef), leaf(fixed), leaf(Xg), leaf(Yg)
    Z = coef_map(w, c, t, gx, gy, xp=tb, **kw)
    ct = torch.ones_like(Z) if cotangent is None else tb.asarray(np.asarray(cotangent))
    gw, gt, gc = torch.autograd.grad((Z * ct).sum(), [w, t, c], retain_graph=True, allow_unused=True)
    ggx, ggy = torch.autograd.grad(Z.sum(), [gx, gy], allow_unused=True)
    z = lambda g, ref: (torch.zeros_like(ref) if g is None else g).detach().numpy()
    return {"value": Z.detach().numpy(), "grad_rx": np.stack([z(ggx, gx), z(ggy, gy)], axis=-1), "tx_bar": z(gt, t),
            "walls_bar": z(gw, w), "coef_bar": z(gc, c)}
