"""Dormand-Prince 5(4) with scipy's step control, the arithmetic on a backend (device-resident RK45 for `sample_mode: continuous`).

The reference integrates the probability-flow ODE with `torchdiffeq.odeint(method="scipy_solver", options={"solver": "RK45"})`
(diffusion/diffusion_continuous.py:88-131), i.e. scipy's `solve_ivp(method="RK45")` on the host.  `rk45_solve` restates scipy
1.15's `RK45` (scipy/integrate/_ivp/rk.py: `rk_step`, `RungeKutta._step_impl`, `_estimate_error_norm`; common.py:
`select_initial_step`, `validate_tol`; base.py: `OdeSolver.step`) with the step control in float64 Python scalars and every pass over
the state handed to a backend, so that the state and the stage derivatives never leave the device:

    backend.stage(y, ks, coefs, h, y_out, x_out)        y_out = y + h * (((a0 k0 + a1 k1) + a2 k2) + ...),  x_out = float32(y_out)
    backend.rhs(x, p, f, g2, sd, k_out, is_score)       k_out = float64(-(f x - (0.5 g2) score)),  score = -p / sd  (or p itself)
    backend.scaled_sumsq(vs, coefs, ya, yb, atol, rtol) sum_i ((sum_j c_j v_j[i]) / (atol + rtol max(|ya[i]|, |yb[i]|)))^2  -> float

`HipBackend` runs them as the kernels of csrc/ode_rk45.hip (device tensors; `scaled_sumsq` is the one 8-byte readback per step
attempt), `NumpyBackend` performs the same operations in the same order on host arrays (CPU tests; the kernels' reference).  The
two differ only in the summation order inside `scaled_sumsq`.  `rhs` is not called by the solver itself: the caller's `fun` uses it
to turn a Score evaluation into a stage derivative (DiffusionBase.sample_model_ode).

What differs from scipy, deliberately: the stage combination is formed left to right (scipy: `np.dot(K[:s].T, a[:s])`, in BLAS's
order), the error norm is |h| norm(sum_j E_j K_j / scale) (scipy: norm(np.dot(K.T, E) * h / scale)), and the state returned is
`y_new` of the last step (solve_ivp with `t_eval` returns the dense output there, the same value up to rounding).  All are
rounding-level: against `solve_ivp` the restatement takes the same steps (tests/test_ode_host.py).
"""
import math

import numpy as np
from scipy.integrate import RK45 as _RK45

A = [[float(v) for v in row] for row in _RK45.A]          # [6][5]; row s combines K[0..s-1] into stage s
B = [float(v) for v in _RK45.B]                           # [6]
C = [float(v) for v in _RK45.C]                           # [6]
E = [float(v) for v in _RK45.E]                           # [7]
N_STAGES = 6
ERROR_EXPONENT = -1.0 / (_RK45.error_estimator_order + 1)  # -1/5
SAFETY = 0.9
MIN_FACTOR = 0.2
MAX_FACTOR = 10.0
TOO_SMALL_STEP = "Required step size is less than spacing between numbers."   # OdeSolver.TOO_SMALL_STEP


class StepSizeTooSmall(RuntimeError):
    """The controller asked for a step below 10 ulp of t (scipy: `solve_ivp` returns status -1 with TOO_SMALL_STEP)."""


class NumpyBackend:
    """Host arrays; one numpy operation per rounding, in the kernels' order."""
    name = "numpy"

    def empty(self, n, dtype):
        return np.empty(n, dtype=dtype)

    def stage(self, y, ks, coefs, h, y_out, x_out):
        acc = np.float64(coefs[0]) * ks[0]
        for c, k in zip(coefs[1:], ks[1:]):
            acc = acc + np.float64(c) * k
        y_out[:] = y + np.float64(h) * acc
        x_out[:] = y_out.astype(np.float32)

    def rhs(self, x, p, f, g2, sd, k_out, is_score=False):
        x, p = np.asarray(x, dtype=np.float32).reshape(-1), np.asarray(p, dtype=np.float32).reshape(-1)
        score = p if is_score else (-p) / np.float32(sd)
        a = np.float32(f) * x
        b = (np.float32(0.5) * np.float32(g2)) * score
        k_out[:] = (-(a - b)).astype(np.float64)

    def scaled_sumsq(self, vs, coefs, ya, yb, atol, rtol):
        e = np.float64(coefs[0]) * vs[0]
        for c, v in zip(coefs[1:], vs[1:]):
            e = e + np.float64(c) * v
        scale = np.float64(atol) + np.float64(rtol) * np.maximum(np.abs(ya), np.abs(yb))
        q = e / scale
        return float(np.sum(q * q))


class HipBackend:
    """Device tensors through ldt_ode_stage / ldt_ode_rhs / ldt_ode_scaled_sumsq (no CPU fallback: a host tensor raises)."""
    name = "hip"

    def __init__(self, device):
        import torch
        from . import _lib
        self.device = torch.device(device)
        self._scratch = torch.empty(_lib.ODE_SUMSQ_SCRATCH, dtype=torch.float64, device=self.device)
        self._out = torch.empty(1, dtype=torch.float64, device=self.device)

    def empty(self, n, dtype):
        import torch
        return torch.empty(n, dtype=torch.float64 if np.dtype(dtype) == np.float64 else torch.float32, device=self.device)

    def stage(self, y, ks, coefs, h, y_out, x_out):
        from . import ops
        ops.ode_stage(y, ks, coefs, h, y_out=y_out, x_out=x_out)

    def rhs(self, x, p, f, g2, sd, k_out, is_score=False):
        from . import ops
        ops.ode_rhs(x.reshape(-1), p.reshape(-1), f, g2, sd, k_out=k_out, is_score=is_score)

    def scaled_sumsq(self, vs, coefs, ya, yb, atol, rtol):
        from . import ops
        ops.ode_scaled_sumsq(vs, coefs, ya, yb, atol, rtol, scratch=self._scratch, out=self._out)
        return float(self._out.item())                     # the readback: 8 bytes, one synchronisation per step attempt


def _rms(sumsq, n):
    return math.sqrt(sumsq) / n ** 0.5                     # scipy's norm(x) = np.linalg.norm(x) / x.size ** 0.5


def select_initial_step(backend, fun, t0, y0, f0, f1, y1, x1, t_bound, max_step, direction, order, rtol, atol):
    """scipy's select_initial_step (Hairer, Norsett, Wanner I, II.4): one Euler probe, hence one evaluation of `fun` (into `f1`;
    `y1` / `x1` are scratch).  -> h_abs."""
    n = int(y0.shape[0])
    interval_length = abs(t_bound - t0)
    if interval_length == 0.0:
        return 0.0
    d0 = _rms(backend.scaled_sumsq([y0], [1.0], y0, y0, atol, rtol), n)
    d1 = _rms(backend.scaled_sumsq([f0], [1.0], y0, y0, atol, rtol), n)
    if d0 < 1e-5 or d1 < 1e-5:
        h0 = 1e-6
    else:
        h0 = 0.01 * d0 / d1
    h0 = min(h0, interval_length)
    backend.stage(y0, [f0], [1.0], h0 * direction, y1, x1)
    fun(t0 + h0 * direction, x1, f1)
    d2 = _rms(backend.scaled_sumsq([f1, f0], [1.0, -1.0], y0, y0, atol, rtol), n) / h0
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1, d2)) ** (1 / (order + 1))
    return min(100 * h0, h1, interval_length, max_step)


def next_factor(error_norm, step_rejected):
    """The step-size factor after an ACCEPTED attempt (error_norm < 1): MAX_FACTOR at zero error, no growth after a rejection."""
    if error_norm == 0:
        factor = MAX_FACTOR
    else:
        factor = min(MAX_FACTOR, SAFETY * error_norm ** ERROR_EXPONENT)
    if step_rejected:
        factor = min(1, factor)
    return factor


def rk45_solve(backend, fun, y0, x0, t0, t_bound, rtol, atol, max_step=math.inf, factors=None):
    """Integrate dy/dt = fun from t0 to t_bound with RK45 as `solve_ivp(method="RK45", rtol=, atol=)` steps it.

    fun(t, x, k_out): writes the derivative at time t into the float64 vector `k_out`, given the float32 cast `x` of the state —
    the cast every evaluation of the host path makes (`torch.from_numpy(y).to(dev, torch.float32)`).
    y0 float64 [n] and x0 = float32(y0), both backend vectors (not modified).  factors: a list that receives, per attempt,
    (accepted, error_norm, factor) — for tests.
    -> (y, nfe, accepted, rejected, t_trace): the state at t_bound (a backend vector), the number of `fun` calls, the step counts
    and the accepted times, t0 first.  Raises StepSizeTooSmall where solve_ivp would return status -1."""
    n = int(y0.shape[0])
    eps = np.finfo(np.float64).eps
    rtol = max(float(rtol), 100 * eps)                     # validate_tol
    atol = float(atol)
    if atol < 0:
        raise ValueError("`atol` must be positive.")
    t, t_bound = float(t0), float(t_bound)
    direction = float(np.sign(t_bound - t)) if t_bound != t else 1.0
    f64 = lambda: backend.empty(n, np.float64)
    K = [f64() for _ in range(N_STAGES + 1)]
    y, y_new, y_s = y0, f64(), f64()
    x = backend.empty(n, np.float32)
    fun(t, x0, K[0])
    nfe = 1
    h_abs = select_initial_step(backend, fun, t, y, K[0], K[1], y_s, x, t_bound, max_step, direction, _RK45.error_estimator_order,
                                rtol, atol)
    nfe += 1
    accepted = rejected = 0
    t_trace = [t]
    while direction * (t - t_bound) < 0:                   # OdeSolver.step until status == "finished"
        min_step = 10 * abs(np.nextafter(t, direction * np.inf) - t)
        if h_abs > max_step:
            h_abs = max_step
        elif h_abs < min_step:
            h_abs = min_step
        step_accepted = step_rejected = False
        while not step_accepted:
            if h_abs < min_step:
                raise StepSizeTooSmall("%s (t = %.17g, h = %.17g, after %d accepted and %d rejected steps)"
                                       % (TOO_SMALL_STEP, t, h_abs * direction, accepted, rejected))
            h = h_abs * direction
            t_new = t + h
            if direction * (t_new - t_bound) > 0:
                t_new = t_bound
            h = t_new - t
            h_abs = abs(h)
            for s in range(1, N_STAGES):                   # rk_step
                backend.stage(y, K[:s], A[s][:s], h, y_s, x)
                fun(t + C[s] * h, x, K[s])
            backend.stage(y, K[:N_STAGES], B, h, y_new, x)
            fun(t + h, x, K[N_STAGES])
            nfe += N_STAGES
            # scipy: norm((np.dot(K.T, E) * h) / scale).  E is passed unscaled and |h| applied to the norm: E sums to zero and the
            # estimate is what survives that cancellation, so coefficients h * E_j — each rounded on its own — would leave a residue
            # of ~1e-16 h |K| in it; through the fp32 cast of the next evaluation times that moved whole step sequences by up to
            # 1e-5 in t against scipy (measured on the cases of tests/test_ode_host.py), where this form stays within 1e-9.
            error_norm = abs(h) * _rms(backend.scaled_sumsq(K, E, y, y_new, atol, rtol), n)
            if error_norm < 1:
                factor = next_factor(error_norm, step_rejected)
                h_abs *= factor
                step_accepted = True
                accepted += 1
            else:                                          # (a NaN norm lands here too and shrinks the step until it is too small)
                factor = max(MIN_FACTOR, SAFETY * error_norm ** ERROR_EXPONENT)
                h_abs *= factor
                step_rejected = True
                rejected += 1
            if factors is not None:
                factors.append((step_accepted, error_norm, factor))
        t = t_new
        if y is y0:                                        # the caller's vector is never written
            y, y_new = y_new, f64()
        else:
            y, y_new = y_new, y
        K[0], K[N_STAGES] = K[N_STAGES], K[0]              # FSAL: f_new is the next step's first stage
        t_trace.append(t)
    return y, nfe, accepted, rejected, t_trace
