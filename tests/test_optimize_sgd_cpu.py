"""
SGD on the host (differt2d_amd.optimize.sgd, optax 0.2.4's optax.sgd): minimize's fp32 update against the closed form of a
quadratic and against a NumPy restatement of optax.sgd / trace / scale_by_learning_rate; the spec's validation; the path
classes' keyword parsing.  The GPU side (the solver kernels and the gradients through them) is tests/test_gpu_opt_sgd.py.
"""

import numpy as np
import pytest

F = np.float32
A = np.array([1.0, -2.0, 0.5, 3.25], F)


def _quadratic(x):
    d = x - A
    return np.dot(d, d)


def _restated_sgd(x0, steps, lr, momentum, nesterov):
    """optax.sgd in fp32: chain(trace(momentum, nesterov), scale(-lr)) -- or scale(-lr) alone for momentum None -- on
    f = |x - a|^2 (gradient 2 (x - a)); the hyper-parameters are weakly typed Python floats (rounded to fp32 where they meet
    an fp32 array).  Returns (x, loss before the last update)."""
    x = np.array(x0, F)
    trace = np.zeros_like(x)
    loss = None
    for _ in range(steps):
        d = x - A
        loss = np.dot(d, d)
        g = F(2.0) * d
        if momentum is None:
            u = g
        else:
            trace = g + F(momentum) * trace
            u = g + F(momentum) * trace if nesterov else trace
        x = x + F(-lr) * u
    return x, loss


@pytest.mark.parametrize("steps", [1, 5, 30])
@pytest.mark.parametrize("lr", [0.1, 0.03])
def test_plain_sgd_follows_the_closed_form(steps, lr):
    """x_t = a + (1 - 2 lr)^t (x0 - a) for f = |x - a|^2: the fp32 iterate within a few ulps of the exact one."""
    from differt2d_amd.optimize import minimize, sgd

    x0 = np.zeros(4, F)
    x, loss = minimize(_quadratic, x0, steps=steps, optimizer=sgd(lr))
    assert x.dtype == F
    r = 1.0 - 2.0 * float(F(lr))
    want = A.astype(np.float64) + r**steps * (x0.astype(np.float64) - A)
    ulp = np.spacing(np.abs(want).astype(F)).astype(np.float64)
    assert (np.abs(x - want) <= 4 * ulp).all(), (x, want, np.abs(x - want) / ulp)
    # the loss is the one evaluated before the last update
    prev = minimize(_quadratic, x0, steps=steps - 1, optimizer=sgd(lr))[0] if steps > 1 else x0
    assert F(loss) == _quadratic(prev)


@pytest.mark.parametrize("momentum,nesterov", [(None, False), (None, True), (0.0, False), (0.5, False), (0.9, False), (0.9, True), (0.3, True)])
def test_sgd_matches_the_numpy_restatement_bit_for_bit(momentum, nesterov):
    from differt2d_amd.optimize import minimize, sgd

    x0 = np.array([0.3, 0.1, -0.7, 2.0], F)
    x, loss = minimize(_quadratic, x0, steps=40, optimizer=sgd(0.05, momentum=momentum, nesterov=nesterov))
    want_x, want_loss = _restated_sgd(x0, 40, 0.05, momentum, nesterov)
    assert np.array_equal(x, want_x) and F(loss) == F(want_loss)


def test_momentum_and_nesterov_change_the_trajectory():
    from differt2d_amd.optimize import minimize, sgd

    x0 = np.zeros(4, F)
    runs = [minimize(_quadratic, x0, steps=10, optimizer=o)[0] for o in (sgd(0.05), sgd(0.05, 0.9), sgd(0.05, 0.9, nesterov=True))]
    assert not np.array_equal(runs[0], runs[1]) and not np.array_equal(runs[1], runs[2])
    # Nesterov without momentum is plain SGD (optax ignores the flag when there is no trace)
    assert np.array_equal(minimize(_quadratic, x0, steps=10, optimizer=sgd(0.05, nesterov=True))[0], runs[0])


def test_sgd_through_the_random_start_utilities():
    from differt2d_amd.optimize import minimize_many_random_uniform, minimize_random_uniform, sgd
    from differt2d_amd.random import PRNGKey

    def f(x):
        d = x - 1.0
        return np.dot(d, d)

    x, y = minimize_random_uniform(f, PRNGKey(1234), 10, optimizer=sgd(0.1))
    assert np.allclose(x, 1.0, rtol=1e-2) and abs(y) <= 1e-4
    x, y = minimize_many_random_uniform(f, PRNGKey(1234), 10, many=3, optimizer=sgd(0.1, momentum=0.5, nesterov=True))
    assert np.allclose(x, 1.0, rtol=1e-2) and abs(y) <= 1e-4


@pytest.mark.parametrize("momentum", [-0.1, 1.0, 1.5, float("nan"), float("inf")])
def test_invalid_momentum_is_refused(momentum):
    from differt2d_amd.optimize import sgd

    with pytest.raises(ValueError):
        sgd(0.1, momentum=momentum)


@pytest.mark.parametrize("lr", [float("nan"), float("inf"), -float("inf")])
def test_a_learning_rate_that_is_not_finite_is_refused(lr):
    from differt2d_amd.optimize import sgd

    with pytest.raises(ValueError):
        sgd(lr)


def test_sgd_spec_mirrors_optax_sgd_arguments():
    from differt2d_amd.optimize import SGD, sgd

    assert sgd() == SGD(0.1, None, False)
    assert sgd(0.02, 0.0) == SGD(0.02, 0.0, False) and sgd(0.02, 0.0) != sgd(0.02)  # momentum 0.0 is not None
    assert sgd(learning_rate=1, momentum=0, nesterov=1) == SGD(1.0, 0.0, True)


def test_path_class_keywords_accept_sgd_and_still_refuse_the_rest():
    from differt2d_amd import _lib as L
    from differt2d_amd.geometry import _opt_kwargs
    from differt2d_amd.optimize import adam, minimize, sgd

    spec = sgd(0.01, momentum=0.9, nesterov=True)
    assert _opt_kwargs(dict(steps=20, optimizer=spec)) == (20, 1, None, spec)
    assert _opt_kwargs(dict(optimizer=sgd(0.2)))[3] == sgd(0.2)
    assert _opt_kwargs(dict(optimizer=adam(0.01)))[3] == adam(0.01)
    for bad in (object(), "sgd"):
        with pytest.raises(L.D2DUnsupported):
            _opt_kwargs(dict(optimizer=bad))
        with pytest.raises(L.D2DUnsupported):
            minimize(_quadratic, np.zeros(4, F), optimizer=bad)
