"""CPU: the RK45 step controller of ldt_amd/ode.py on its numpy backend, held against scipy's own `solve_ivp(method="RK45")`, its
corner cases, and the `sample_model_ode(solver=...)` surface.  No GPU: the backend performs the kernels' operations on host arrays."""
import math

import numpy as np
import pytest
import torch
from scipy.integrate import solve_ivp

from ldt_amd import ode

BETA0, BETA1, SIGMA2_0 = np.float32(0.1), np.float32(20.0), np.float32(1e-4)


def _vp_scalars(t):
    """f, g2, sd of the VP-SDE with beta = (0.1, 20), sigma2_0 = 1e-4 at the fp32 time t, in fp32 (DiffusionVPSDE's operation order)."""
    t = np.float32(t)
    g2 = BETA0 + (BETA1 - BETA0) * t
    f = np.float32(-0.5) * g2
    var = np.float32(1.0) - (np.float32(1.0) - SIGMA2_0) * np.exp(-BETA0 * t - np.float32(0.5) * (BETA1 - BETA0) * t * t, dtype=np.float32)
    return f, g2, np.sqrt(var), var


def _score(kind, x, sd, var):
    if kind == "linear":
        return -x / var
    return -np.tanh(np.float32(3.0) * x) / sd


def _rhs_fp32(kind, s, x):
    """The reversed-time right-hand side in fp32 on the fp32 state x, as the real path evaluates it."""
    f, g2, sd, var = _vp_scalars(-s)
    dx = f * x - (np.float32(0.5) * g2) * _score(kind, x, sd, var)
    return (-dx).astype(np.float64)


def _run_both(kind, n, tol):
    y0 = np.random.default_rng(n + 17).standard_normal(n).astype(np.float32).astype(np.float64)
    sol = solve_ivp(lambda s, y: _rhs_fp32(kind, s, y.astype(np.float32)), t_span=[-1.0, -1e-2], y0=y0, method="RK45", rtol=tol, atol=tol)
    assert sol.status == 0

    def fun(s, x, k_out):
        k_out[:] = _rhs_fp32(kind, s, x)

    y, nfe, acc, rej, trace = ode.rk45_solve(ode.NumpyBackend(), fun, y0, y0.astype(np.float32), -1.0, -1e-2, tol, tol)
    rel = float(((y - sol.y[:, -1]) ** 2).sum() / (sol.y[:, -1] ** 2).sum())
    dt = float(np.abs(np.asarray(trace) - sol.t).max()) if len(trace) == len(sol.t) else math.inf
    print("ode host %-6s n=%-6d tol=%g: nfe %d / scipy %d, accepted %d / %d, rejected %d, max |dt| %.2e, rel-MSE %.2e"
          % (kind, n, tol, nfe, sol.nfev, acc, len(sol.t) - 1, rej, dt, rel))
    return sol, y, nfe, acc, rej, trace, dt, rel


@pytest.mark.parametrize("tol", [1e-3, 1e-5])
@pytest.mark.parametrize("n", [256, 245760])
@pytest.mark.parametrize("kind", ["linear", "tanh"])
def test_controller_takes_scipys_steps(kind, n, tol):
    sol, y, nfe, acc, rej, trace, dt, rel = _run_both(kind, n, tol)
    assert nfe == sol.nfev == 2 + 6 * (acc + rej)
    assert acc == len(sol.t) - 1
    assert dt <= 1e-6
    assert rel <= 1e-12


@pytest.mark.parametrize("n", [256, 245760])
@pytest.mark.parametrize("kind", ["linear", "tanh"])
def test_controller_at_1e_7_same_work_and_state(kind, n):
    """At tol = 1e-7 the fp32 right-hand side's rounding noise is of the size of the error estimate, so the two time grids drift
    apart (by ~2e-4); the work and the result still agree."""
    sol, y, nfe, acc, rej, trace, dt, rel = _run_both(kind, n, 1e-7)
    assert nfe == sol.nfev
    assert rel <= 1e-10


def test_tableaux_are_scipys():
    from scipy.integrate import RK45
    assert np.array_equal(np.asarray(ode.A), RK45.A) and np.array_equal(np.asarray(ode.B), RK45.B)
    assert np.array_equal(np.asarray(ode.C), RK45.C) and np.array_equal(np.asarray(ode.E), RK45.E)
    assert ode.ERROR_EXPONENT == -0.2 and (ode.SAFETY, ode.MIN_FACTOR, ode.MAX_FACTOR) == (0.9, 0.2, 10.0)


def _solve(fun, y0, t0=0.0, t1=1.0, tol=1e-6, **kw):
    y0 = np.asarray(y0, dtype=np.float64)
    return ode.rk45_solve(ode.NumpyBackend(), fun, y0, y0.astype(np.float32), t0, t1, tol, tol, **kw)


def test_no_growth_after_a_rejection_and_last_step_lands_on_t_bound():
    def fun(t, x, k_out):                                   # a sharp feature in the middle of the interval forces rejections
        k_out[:] = 1.0 / (1e-4 + (t - 0.5) ** 2) * np.cos(x.astype(np.float64))
    factors = []
    y, nfe, acc, rej, trace = _solve(fun, np.zeros(8), factors=factors)
    assert rej > 0 and acc + rej == len(factors) and nfe == 2 + 6 * len(factors)
    after_reject = [factors[i + 1] for i in range(len(factors) - 1) if not factors[i][0]]
    assert after_reject
    for ok, err, fac in after_reject:                       # accepted: min(1, .) ; rejected again: max(0.2, 0.9 err^-0.2) < 1
        assert fac <= 1
    for ok, err, fac in factors:
        assert ok == (err < 1) and ode.MIN_FACTOR <= fac <= ode.MAX_FACTOR
    assert trace[0] == 0.0 and trace[-1] == 1.0 and len(trace) == acc + 1
    assert all(b > a for a, b in zip(trace, trace[1:]))


def test_backward_integration_lands_on_t_bound():
    def fun(t, x, k_out):
        k_out[:] = -x.astype(np.float64)
    y, nfe, acc, rej, trace = _solve(fun, np.ones(4), t0=1.0, t1=-0.25)
    assert trace[-1] == -0.25 and all(b < a for a, b in zip(trace, trace[1:]))
    assert np.allclose(y, math.exp(1.25), rtol=1e-5)


def test_zero_error_takes_max_factor():
    def fun(t, x, k_out):                                   # a zero derivative: every stage is exactly zero, so error_norm == 0
        k_out[:] = 0.0
    factors = []
    y, nfe, acc, rej, trace = _solve(fun, np.full(4, 200.0), t1=100.0, factors=factors)
    assert rej == 0 and all(f == (True, 0.0, ode.MAX_FACTOR) for f in factors)
    assert ode.next_factor(0.0, False) == ode.MAX_FACTOR and ode.next_factor(0.0, True) == 1
    assert ode.next_factor(0.5, True) == 1 and ode.next_factor(0.999, False) < 1 < ode.next_factor(0.5, False)
    assert np.array_equal(y, np.full(4, 200.0))


def test_step_below_min_step_raises_like_scipys_status_minus_one():
    def fun(t, x, k_out):                                   # 1 / (1 - t): no step gets past the pole at t = 1
        k_out[:] = x.astype(np.float64) ** 2
    sol = solve_ivp(lambda t, y: y.astype(np.float32).astype(np.float64) ** 2, [0.0, 2.0], np.ones(2), method="RK45", rtol=1e-6, atol=1e-6)
    assert sol.status == -1 and sol.message == ode.TOO_SMALL_STEP
    with pytest.raises(ode.StepSizeTooSmall, match=r"Required step size is less than spacing between numbers.*t = .*h = ") as ei:
        _solve(fun, np.ones(2), t1=2.0)
    assert isinstance(ei.value, RuntimeError)

    def nan_fun(t, x, k_out):                               # a NaN error norm is a rejection, then a too small step (as scipy)
        k_out[:] = np.nan if t > 0.5 else 1.0
    with pytest.raises(ode.StepSizeTooSmall):
        _solve(nan_fun, np.zeros(2))


def test_numpy_backend_operations():
    """The backend's three operations against their definitions written out (they are the reference the kernel tests use)."""
    rng = np.random.default_rng(3)
    be = ode.NumpyBackend()
    y, ks = rng.standard_normal(50), [rng.standard_normal(50) for _ in range(6)]
    a = list(rng.standard_normal(6))
    yo, xo = np.empty(50), np.empty(50, dtype=np.float32)
    be.stage(y, ks[:3], a[:3], 0.37, yo, xo)
    assert np.array_equal(yo, y + 0.37 * ((a[0] * ks[0] + a[1] * ks[1]) + a[2] * ks[2])) and np.array_equal(xo, yo.astype(np.float32))
    x, p = rng.standard_normal(50).astype(np.float32), rng.standard_normal(50).astype(np.float32)
    f, g2, sd = np.float32(-3.1), np.float32(6.2), np.float32(0.7)
    ko = np.empty(50)
    be.rhs(x, p, f, g2, sd, ko)
    assert ko.dtype == np.float64 and np.array_equal(ko, (-(f * x - (np.float32(0.5) * g2) * (-p / sd))).astype(np.float64))
    be.rhs(x, p, f, g2, sd, ko, is_score=True)
    assert np.array_equal(ko, (-(f * x - (np.float32(0.5) * g2) * p)).astype(np.float64))
    yb = rng.standard_normal(50)
    got = be.scaled_sumsq(ks[:2], [1.0, -1.0], y, yb, 1e-3, 1e-2)
    want = (((ks[0] - ks[1]) / (1e-3 + 1e-2 * np.maximum(np.abs(y), np.abs(yb)))) ** 2).sum()
    assert abs(got - want) <= 1e-14 * want


def _sde():
    import ldt_amd
    from ldt_amd.diffusion import DiffusionVPSDE
    return DiffusionVPSDE(ldt_amd.airplane_config(latent_tokens=8).sde)


def test_sample_model_ode_solver_surface():
    sde = _sde()
    fn = lambda t, x, label=None, condition=None: (x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sde.sample_model_ode(fn, 2, (8, 4), 1e-2, 1e-3, device="cpu", solver="device")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sde.sample_model_ode(fn, 2, (8, 4), 1e-2, 1e-3, device="cpu")
    for dev in ("cpu", "cuda"):
        with pytest.raises(ValueError, match="solver"):
            sde.sample_model_ode(fn, 2, (8, 4), 1e-2, 1e-3, device=dev, solver="rk23")


def test_config_default_and_binding():
    import ldt_amd
    from ldt_amd import _lib
    assert ldt_amd.airplane_config().sde.ode_solver == "scipy"
    for name in ("ldt_ode_stage", "ldt_ode_rhs", "ldt_ode_scaled_sumsq"):
        assert name in _lib.SIGNATURES


def test_ode_entry_points_return_argument_errors():
    """Null pointers, a zero or odd n and a bad term count come back as a status with a message (no launch, so no GPU needed)."""
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib
    lib = _lib.lib()
    z6, z7 = [0.0] * 6, [0.0] * 7
    keep = np.zeros(64)
    buf = (keep.ctypes.data + 15) // 16 * 16                     # a non-null aligned address: no call below gets as far as a launch
    assert lib.ldt_ode_stage(None, *([None] * 6), *z6, 1, 0.1, None, None, 8, None) == -1 and b"null" in lib.ldt_last_error()
    assert lib.ldt_ode_stage(buf, buf, *([None] * 5), *z6, 2, 0.1, buf, buf, 8, None) == -1 and b"K1 of 2" in lib.ldt_last_error()
    assert lib.ldt_ode_stage(buf, buf, *([None] * 5), *z6, 0, 0.1, buf, buf, 8, None) == -1 and b"nterms" in lib.ldt_last_error()
    for n in (0, 7, -2):
        assert lib.ldt_ode_stage(buf, buf, *([None] * 5), *z6, 1, 0.1, buf, buf, n, None) == -2 and b"multiple of 2" in lib.ldt_last_error()
        assert lib.ldt_ode_rhs(buf, buf, 0, 0.0, 1.0, 1.0, buf, n, None) == -2 and b"multiple of 2" in lib.ldt_last_error()
        assert lib.ldt_ode_scaled_sumsq(buf, *([None] * 6), *z7, 1, buf, buf, 1e-3, 1e-3, buf, 1024, buf, n, None) == -2
        assert b"multiple of 2" in lib.ldt_last_error()
    assert lib.ldt_ode_stage(buf, buf + 8, *([None] * 5), *z6, 1, 0.1, buf, buf, 8, None) == -3 and b"aligned" in lib.ldt_last_error()
    assert lib.ldt_ode_rhs(None, buf, 0, 0.0, 1.0, 1.0, buf, 8, None) == -1 and b"null" in lib.ldt_last_error()
    assert lib.ldt_ode_rhs(buf, buf, 0, 0.0, 1.0, 0.0, buf, 8, None) == -1 and b"sd" in lib.ldt_last_error()
    assert lib.ldt_ode_scaled_sumsq(buf, *([None] * 6), *z7, 1, buf, buf, 1e-3, 1e-3, None, 1024, buf, 8, None) == -1
    assert lib.ldt_ode_scaled_sumsq(buf, *([None] * 6), *z7, 8, buf, buf, 1e-3, 1e-3, buf, 1024, buf, 8, None) == -1 and b"nvec" in lib.ldt_last_error()
    assert lib.ldt_ode_scaled_sumsq(buf, *([None] * 6), *z7, 1, buf, buf, 1e-3, 1e-3, buf, 0, buf, 8, None) == -1 and b"scratch_len" in lib.ldt_last_error()
    assert lib.ldt_ode_scaled_sumsq(buf, *([None] * 6), *z7, 1, buf, buf, 0.0, 0.0, buf, 1024, buf, 8, None) == -1 and b"atol" in lib.ldt_last_error()
