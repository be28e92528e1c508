"""GPU (-m gpu): the device-resident RK45 of `sample_mode: continuous` — the three kernels of csrc/ode_rk45.hip per element, the
controller on the HIP backend against the same controller on the numpy backend, and `sample_model_ode(solver="device")` /
`Trainer.sample` end to end against the oracle and the scipy path.

Yardsticks: the kernels do one correctly rounded IEEE operation per step of a stated expression, so `ldt_ode_stage` and
`ldt_ode_rhs` are held to `torch.equal` with that expression evaluated by torch on the CPU; the norm is a sum of non-negative
terms, so any summation order lies within n 2^-53 relative of any other.  End to end the bar is the project's own for this mode,
rel-MSE < 1e-3: both solvers are adaptive and see a bf16 Score."""
import copy
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_mse

pytestmark = pytest.mark.gpu

TINY_N = 2 * 8 * 120                        # B x tokens x z of the tiny fixture
SIZES = [8, 250, TINY_N, 1966080]           # 250 and 1920 are not multiples of a workgroup's span (256 threads x 2 elements)
PAD = 4                                     # elements of NaN / sentinel on either side: keeps every slice 16-byte aligned
SENTINEL = -7777.25


def _wrapped(v):
    """`v` (1-d, CPU) inside a NaN-filled device buffer -> the device view of it."""
    buf = torch.full((v.numel() + 2 * PAD,), float("nan"), dtype=v.dtype, device="cuda")
    buf[PAD:PAD + v.numel()] = v.cuda()
    return buf[PAD:PAD + v.numel()]


def _out(n, dtype):
    """A sentinel-filled device buffer and its [n] interior view."""
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n]


def _margins_intact(buf):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())


def _sde(kind):
    import ldt_amd
    base = dict(sigma2_0=1e-4, time_eps=0.01, sample_time_eps=1e-2, beta_start=0.1, beta_end=20.0, train_N=1000, sample_mode="continuous")
    if kind == 0:
        return ldt_amd.make_diffusion(SimpleNamespace(sde_type="vpsde", **base))
    if kind == 1:
        return ldt_amd.make_diffusion(SimpleNamespace(sde_type="sub_vpsde", **base))
    return ldt_amd.make_diffusion(SimpleNamespace(sde_type="vesde", sigma2_min=1e-4, sigma2_max=36.0, **base))


def _host_scalars(sde, t):
    """f, g2, sd at the fp32 time t exactly as `_sample_model_ode_device` forms them."""
    th = torch.tensor(float(t), dtype=torch.float32)
    return float(sde.f(th)), float(sde.g2(th)), float(torch.sqrt(sde.var(th)))


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("n", SIZES)
def test_ode_stage_kernel_exact(n):
    from ldt_amd import ode, ops
    g = torch.Generator().manual_seed(n)
    y = torch.randn(n, dtype=torch.float64, generator=g)
    ks = [torch.randn(n, dtype=torch.float64, generator=g) * (1.0 + s) for s in range(6)]
    yd, kd = _wrapped(y), [_wrapped(k) for k in ks]
    cases = [([1.0], 1.7e-3)] + [(ode.A[s][:s], -0.0371) for s in range(1, 6)] + [(ode.B, 0.0371)]   # Euler probe, stages 1-5, y_new
    for coefs, h in cases:
        nt = len(coefs)
        acc = coefs[0] * ks[0]
        for c, k in zip(coefs[1:], ks[1:nt]):
            acc = acc + c * k
        want = y + h * acc
        ybuf, yo = _out(n, torch.float64)
        xbuf, xo = _out(n, torch.float32)
        ops.ode_stage(yd, kd[:nt], coefs, h, y_out=yo, x_out=xo)
        torch.cuda.synchronize()
        assert torch.equal(yo.cpu(), want), (n, nt)
        assert torch.equal(xo.cpu(), want.float()), (n, nt)
        assert _margins_intact(ybuf) and _margins_intact(xbuf)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_ode_rhs_kernel_exact(n, kind):
    """K = double(-(f x - 0.5 g2 score)) against fun()'s own torch expression (DiffusionBase.sample_model_ode) fed by
    ops.sde_score, for the three score kinds.  Every operation is one correctly rounded IEEE fp32 operation: the library is built
    without fast-math and hipcc's fp32 division is the correctly rounded one by default, so the comparison is exact.
    The kernel takes sd = sqrt(var(t)) from the host where ldt_sde_score evaluates var(t) itself (expf / powf on the device): the
    comparison fed by ops.sde_score is made at t = 1, where var does not depend on the last bit of the exponential (e ~ 4e-5
    against var ~ 1; pow(r, 1) = r) — that the two agree there is asserted first.  Other times are checked with the score formed
    by the same expression on the CPU from the host's sd."""
    from ldt_amd import ops
    sde = _sde(kind)
    g = torch.Generator().manual_seed(7 * n + kind)
    x = torch.randn(n, generator=g) * 3.0
    p = torch.randn(n, generator=g)
    xd, pd = _wrapped(x), _wrapped(p)

    def check(t, score, is_score):
        f, g2, sd = _host_scalars(sde, t)
        tt = torch.full((1,), float(t), dtype=torch.float32)
        if score is None:
            score = -p / torch.tensor(sd, dtype=torch.float32)
        dx = sde.f(tt)[:, None] * x[None] - 0.5 * sde.g2(tt)[:, None] * score[None]          # diffusion.py fun(), on the CPU
        want = (-dx).reshape(-1).double()
        kbuf, ko = _out(n, torch.float64)
        ops.ode_rhs(xd, _wrapped(score) if is_score else pd, f, g2, sd, k_out=ko, is_score=is_score)
        torch.cuda.synchronize()
        assert torch.equal(ko.cpu(), want), (n, kind, t, is_score)
        assert _margins_intact(kbuf)

    if n % 4 == 0:                                         # ldt_sde_score wants rows of a multiple of 4
        t1 = torch.ones(1, device="cuda")
        score_dev = ops.sde_score(pd.view(1, n), t1, sde.score_kind, *sde.score_consts()).view(-1).cpu()
        assert torch.equal(score_dev, -p / torch.tensor(_host_scalars(sde, 1.0)[2], dtype=torch.float32)), "host sd != kernel sd at t = 1"
        check(1.0, score_dev, False)
        check(1.0, score_dev, True)                        # the opaque-score entry on the same values
    for t in (1.0, 0.37, 1e-2):
        check(t, None, False)
    check(0.37, torch.randn(n, generator=g), True)


@pytest.mark.parametrize("n", SIZES)
def test_ode_scaled_sumsq_kernel(n):
    from ldt_amd import _lib, ode, ops
    g = torch.Generator().manual_seed(3 * n + 1)
    vs = [torch.randn(n, dtype=torch.float64, generator=g) for _ in range(7)]
    ya, yb = torch.randn(n, dtype=torch.float64, generator=g), torch.randn(n, dtype=torch.float64, generator=g) * 2.0
    vd, yad, ybd = [_wrapped(v) for v in vs], _wrapped(ya), _wrapped(yb)
    scratch = torch.full((_lib.ODE_SUMSQ_SCRATCH + 2 * PAD,), SENTINEL, dtype=torch.float64, device="cuda")
    be = ode.NumpyBackend()
    for coefs, atol, rtol in (([1.0], 1e-3, 1e-3), ([1.0, -1.0], 1e-5, 1e-5), (ode.E, 1e-3, 1e-5)):
        nv = len(coefs)
        want = be.scaled_sumsq([v.numpy() for v in vs[:nv]], coefs, ya.numpy(), yb.numpy(), atol, rtol)
        got = []
        for _ in range(3):
            obuf, out = _out(1, torch.float64)
            ops.ode_scaled_sumsq(vd[:nv], coefs, yad, ybd, atol, rtol, scratch=scratch[PAD:-PAD], out=out)
            got.append(float(out.item()))
            assert _margins_intact(obuf) and _margins_intact(scratch)
        print("ode_scaled_sumsq n=%d nvec=%d: device %.17g numpy %.17g rel %.2e (bound %.2e)"
              % (n, nv, got[0], want, abs(got[0] - want) / want, n * 2.0 ** -53))
        assert got[0] == got[1] == got[2]
        assert abs(got[0] - want) <= n * 2.0 ** -53 * want
    small = torch.empty(3, dtype=torch.float64, device="cuda")          # fewer partial slots than workgroups: the grid is capped, same sum
    out = ops.ode_scaled_sumsq(vd[:1], [1.0], yad, ybd, 1e-3, 1e-3, scratch=small)
    want = be.scaled_sumsq([vs[0].numpy()], [1.0], ya.numpy(), yb.numpy(), 1e-3, 1e-3)
    assert abs(float(out.item()) - want) <= n * 2.0 ** -53 * want


def test_ode_argument_errors_return_a_status():
    from ldt_amd import _lib, ops
    y = torch.zeros(16, dtype=torch.float64, device="cuda")
    x = torch.zeros(16, dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.LdtHipError, match="multiple of 2"):
        ops.ode_stage(y[:7], [y[8:15]], [1.0], 0.1)
    with pytest.raises(_lib.LdtHipError, match="aligned"):
        ops.ode_stage(y[1:9], [y[8:16]], [1.0], 0.1)
    with pytest.raises(_lib.LdtHipError, match="multiple of 2"):
        ops.ode_rhs(x[:7], x[8:15], -1.0, 2.0, 0.5)
    with pytest.raises(_lib.LdtHipError, match="sd"):
        ops.ode_rhs(x[:8], x[8:], -1.0, 2.0, 0.0)
    with pytest.raises(_lib.LdtHipError, match="atol"):
        ops.ode_scaled_sumsq([y[:8]], [1.0], y[:8], y[8:], 0.0, 0.0)
    with pytest.raises(_lib.LdtHipError, match="no CPU fallback"):
        ops.ode_stage(y.cpu(), [y], [1.0], 0.1)
    with pytest.raises(ValueError):
        ops.ode_stage(y, [y] * 7, [1.0] * 7, 0.1)
    with pytest.raises(TypeError):
        ops.ode_rhs(y, x, -1.0, 2.0, 0.5)
    rc = _lib.lib().ldt_ode_rhs(None, None, 0, 0.0, 1.0, 1.0, None, 8, None)
    assert rc == -1 and b"null" in _lib.lib().ldt_last_error()
    torch.cuda.synchronize()                               # and the device is still healthy
    assert float(ops.ode_scaled_sumsq([y[:8] + 1.0], [1.0], y[:8], y[8:], 1.0, 0.0).item()) == 8.0


# ------------------------------------------------------------------------------------------------ controller
def _analytic_params(kind, x):
    """An 'eps prediction' made of correctly rounded operations only, so the CPU and the GPU evaluate it alike: linear (the score of a
    Gaussian) or a rational non-linearity.  torch evaluates each operation as its own kernel: nothing is fused."""
    if kind == "linear":
        return x * 0.75
    return x / (x * x + 1.0) * 2.0


@pytest.mark.parametrize("tol", [1e-3, 1e-5])
@pytest.mark.parametrize("n", [256, 245760])
@pytest.mark.parametrize("kind", ["linear", "rational"])
def test_device_controller_equals_numpy_controller(kind, n, tol):
    from ldt_amd import ode
    sde = _sde(0)
    y0 = torch.randn(n, generator=torch.Generator().manual_seed(n + 5)).double()

    def run(backend, y0v, x0v):
        def fun(s, x, k_out):
            f, g2, sd = _host_scalars(sde, -s)
            backend.rhs(x, _analytic_params(kind, x), f, g2, sd, k_out)
        return ode.rk45_solve(backend, fun, y0v, x0v, -1.0, -1e-2, tol, tol)

    yc, nfe_c, acc_c, rej_c, tr_c = run(ode.NumpyBackend(), y0.numpy(), y0.float().numpy())
    y0d = y0.cuda()
    yd, nfe_d, acc_d, rej_d, tr_d = run(ode.HipBackend("cuda:0"), y0d, y0d.float())
    rel = rel_mse(yd.cpu(), torch.from_numpy(yc))
    dt = max(abs(a - b) for a, b in zip(tr_c, tr_d)) if len(tr_c) == len(tr_d) else math.inf
    print("ode controller %s n=%d tol=%g: nfe %d / %d, accepted %d / %d, rejected %d / %d, max |dt| %.2e, rel-MSE %.2e"
          % (kind, n, tol, nfe_d, nfe_c, acc_d, acc_c, rej_d, rej_c, dt, rel))
    assert nfe_d == nfe_c and acc_d == acc_c
    assert rel <= 1e-12


# ------------------------------------------------------------------------------------------------ end to end, tiny model
@pytest.fixture(scope="module")
def env(tiny_cfg):
    import ldt_amd
    from oracle import ldt_oracle as O
    assert torch.cuda.is_available()
    cfg = copy.deepcopy(tiny_cfg)
    _, ssd = load_golden("score_tiny")
    _, csd = load_golden("trainer_sample_tiny")
    score = ldt_amd.Score(cfg.score)
    score.load_state_dict(ssd["w"], strict=True)
    comp = ldt_amd.Compressor(cfg.compressor)
    comp.load_state_dict(csd["c"], strict=True)
    tr = ldt_amd.Trainer(cfg, score, comp, "cuda:0")
    x1 = torch.randn(2, cfg.score.z_scale, cfg.score.z_dim, generator=torch.Generator().manual_seed(21))
    return dict(ldt=ldt_amd, O=O, tr=tr, ssd=ssd["w"], cfg=cfg, x1=x1)


TOL, EPS = 1e-3, 1e-2


def _scipy_run(tr, monkeypatch, **kw):
    """The scipy path plus its accepted-step count (RK45._step_impl returns once per accepted step)."""
    from scipy.integrate import RK45
    steps = []
    real = RK45._step_impl

    def counting(self):
        r = real(self)
        steps.append(r[0])
        return r
    with monkeypatch.context() as m:
        m.setattr(RK45, "_step_impl", counting)
        out, nfe, secs = tr.SDE.sample_model_ode(tr.score_fn, device="cuda:0", **kw)
    return out, nfe, secs, sum(bool(s) for s in steps)


def test_device_solver_end_to_end_tiny(env, monkeypatch):
    tr, cfg, O, x1 = env["tr"], env["cfg"], env["O"], env["x1"]
    B, T, z = x1.shape
    kw = dict(num_samples=B, shape=(T, z), ode_eps=EPS, ode_solver_tol=TOL, noise=x1)
    dev_s, nfe_s, sec_s = tr.SDE.sample_model_ode(tr.score_fn, device="cuda:0", solver="device", **kw)
    info_s = dict(tr.SDE.last_ode)
    dev_o, nfe_o, sec_o = tr.SDE.sample_model_ode(tr.score_fn, device="cuda:0", solver="device", shared_t=False, **kw)
    info_o = dict(tr.SDE.last_ode)
    dev_t, nfe_t, _ = tr.SDE.sample_model_ode(tr.score_fn, device="cuda:0", solver="device", shared_t=True, **kw)
    assert info_s["route"] == "shared_t" and info_o["route"] == "opaque" and torch.equal(dev_t, dev_s)
    sci, nfe_sci, sec_sci, acc_sci = _scipy_run(tr, monkeypatch, **kw)
    sde = O.VPSDE(cfg.sde)
    fn = O.score_fn_from_model(sde, lambda x, t: O.score_forward(env["ssd"], cfg.score, x, t))
    ref = O.sample_model_ode(sde, fn, x1, EPS, TOL)
    e_oracle, e_scipy, e_routes = rel_mse(dev_s.cpu(), ref), rel_mse(dev_o.cpu(), sci.cpu()), rel_mse(dev_s.cpu(), dev_o.cpu())
    print("ode tiny: device(shared_t) vs oracle %.3e | device(opaque) vs scipy %.3e | shared_t vs opaque %.3e | scipy vs oracle %.3e"
          % (e_oracle, e_scipy, e_routes, rel_mse(sci.cpu(), ref)))
    print("ode tiny: nfe scipy %d, device opaque %d, device shared_t %d; accepted/rejected scipy %d/%d, opaque %d/%d, shared_t %d/%d; "
          "seconds scipy %.3f, opaque %.3f, shared_t %.3f"
          % (nfe_sci, nfe_o, nfe_s, acc_sci, (nfe_sci - 2) // 6 - acc_sci, info_o["accepted"], info_o["rejected"], info_s["accepted"],
             info_s["rejected"], sec_sci, sec_o, sec_s))
    for out, nfe, secs in ((dev_s, nfe_s, sec_s), (dev_o, nfe_o, sec_o)):
        assert out.shape == ref.shape and out.dtype == torch.float32 and out.is_cuda
        assert bool(torch.isfinite(out).all()) and nfe >= 7 and secs > 0
    assert nfe_s == 2 + 6 * (info_s["accepted"] + info_s["rejected"])
    assert info_s["t"][0] == -1.0 and info_s["t"][-1] == -EPS
    assert e_oracle < 1e-3
    assert e_scipy < 1e-3
    assert e_routes < 1e-3
    with pytest.raises(ValueError, match="shared_t"):
        tr.SDE.sample_model_ode(tr.score_fn, device="cuda:0", solver="device", shared_t=True, label=torch.zeros(B, dtype=torch.long), **kw)


def test_trainer_sample_continuous_selects_the_solver(env, monkeypatch):
    import scipy.integrate
    tr, cfg, x1 = env["tr"], env["cfg"], env["x1"]
    B, T, z = x1.shape
    lat_dev, nfe_dev, _ = tr.SDE.sample_model_ode(tr.score_fn, B, (T, z), EPS, TOL, noise=x1, device="cuda:0", solver="device")
    calls = []
    real = scipy.integrate.solve_ivp

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(scipy.integrate, "solve_ivp", counting)
    monkeypatch.delenv("LDT_ODE_SOLVER", raising=False)
    monkeypatch.setattr(tr, "sample_mode", "continuous")
    monkeypatch.setattr(tr, "sample_time_eps", EPS)
    monkeypatch.setattr(cfg.sde, "ode_tol", TOL)
    assert not hasattr(cfg.sde, "ode_solver")                        # the reference's YAMLs carry no such key
    # the configuration
    monkeypatch.setattr(cfg.sde, "ode_solver", "device", raising=False)
    pts, lat = tr.sample(B, x0=x1)
    assert not calls and tr.nfe_count == nfe_dev
    assert rel_mse(lat.cpu(), lat_dev.cpu()) < 1e-6 and pts.shape[0] == B and bool(torch.isfinite(pts).all())
    want_pts = tr.compressor.sample((B, tr.num_points), given_eps=lat_dev)
    assert rel_mse(pts.cpu(), want_pts.cpu()) < 1e-6
    # the environment, when the configuration does not say
    monkeypatch.setattr(cfg.sde, "ode_solver", None, raising=False)
    monkeypatch.setenv("LDT_ODE_SOLVER", "device")
    pts2, lat2 = tr.sample(B, x0=x1)
    assert not calls and tr.nfe_count == nfe_dev
    assert rel_mse(lat2.cpu(), lat_dev.cpu()) < 1e-6 and rel_mse(pts2.cpu(), want_pts.cpu()) < 1e-6
    # neither: the scipy path
    monkeypatch.delenv("LDT_ODE_SOLVER")
    pts3, lat3 = tr.sample(B, x0=x1)
    assert len(calls) == 1 and tr.nfe_count >= 7
    assert rel_mse(lat3.cpu(), lat_dev.cpu()) < 1e-3
    monkeypatch.setenv("LDT_ODE_SOLVER", "rk23")
    with pytest.raises(ValueError, match="solver"):
        tr.sample(B, x0=x1)


def test_conditioned_and_labelled_calls_take_the_opaque_route(env, tiny_cfg):
    import ldt_amd
    tr, cfg, x1 = env["tr"], env["cfg"], env["x1"]
    B, T, z = x1.shape
    a, _ = load_golden("score_tiny")
    cond = (a["pts_cond"][:B].transpose(1, 2).contiguous().cuda(), a["img_cond"][:B].cuda())
    kw = dict(num_samples=B, shape=(T, z), ode_eps=EPS, ode_solver_tol=TOL, noise=x1, device="cuda:0")
    dev, nfe_d, _ = tr.SDE.sample_model_ode(tr.score_fn, condition=cond, solver="device", **kw)
    assert tr.SDE.last_ode["route"] == "opaque"
    sci, nfe_s, _ = tr.SDE.sample_model_ode(tr.score_fn, condition=cond, solver="scipy", **kw)
    plain, _, _ = tr.SDE.sample_model_ode(tr.score_fn, solver="device", **kw)
    e = rel_mse(dev.cpu(), sci.cpu())
    print("ode conditioned: device vs scipy %.3e (nfe %d / %d)" % (e, nfe_d, nfe_s))
    assert bool(torch.isfinite(dev).all()) and e < 1e-3
    assert rel_mse(dev.cpu(), plain.cpu()) > 1e-6                    # and the condition was used
    # labels: a class-conditional Score with seeded weights
    lcfg = copy.deepcopy(tiny_cfg)
    lcfg.score.num_categorys = 5
    lcfg.data.num_categorys = 5
    torch.manual_seed(9)
    ltr = ldt_amd.Trainer(lcfg, ldt_amd.Score(lcfg.score), tr.compressor, "cuda:0")
    label = torch.tensor([4, 1], device="cuda:0")
    dev, nfe_d, _ = ltr.SDE.sample_model_ode(ltr.score_fn, label=label, solver="device", **kw)
    assert ltr.SDE.last_ode["route"] == "opaque"
    sci, nfe_s, _ = ltr.SDE.sample_model_ode(ltr.score_fn, label=label, solver="scipy", **kw)
    e = rel_mse(dev.cpu(), sci.cpu())
    print("ode labelled: device vs scipy %.3e (nfe %d / %d)" % (e, nfe_d, nfe_s))
    assert bool(torch.isfinite(dev).all()) and e < 1e-3

    # a caller's own score_fn: its score is used as given (is_score), as on the scipy path
    def own(t, x, label=None, condition=None):
        return -0.5 * x, None
    dev, _, _ = tr.SDE.sample_model_ode(own, solver="device", **kw)
    sci, _, _ = tr.SDE.sample_model_ode(own, solver="scipy", **kw)
    assert tr.SDE.last_ode["route"] == "opaque" and rel_mse(dev.cpu(), sci.cpu()) < 1e-10


def test_device_solver_at_production_width():
    """hidden 1024 x 24 blocks, seeded weights, B = 4 shapes x 32 tokens (the shipped YAML's token count), tol = 1e-3."""
    import ldt_amd
    cfg = ldt_amd.airplane_config(latent_tokens=32)
    assert (cfg.score.hidden_size, cfg.score.num_blocks) == (1024, 24)
    torch.manual_seed(0)
    score = ldt_amd.Score(cfg.score)
    comp = ldt_amd.Compressor(cfg.compressor)
    tr = ldt_amd.Trainer(cfg, score, comp, "cuda:0")
    tr.model.eval()
    B, T, z = 4, 32, cfg.score.z_dim
    x1 = torch.randn(B, T, z, generator=torch.Generator().manual_seed(4))
    kw = dict(num_samples=B, shape=(T, z), ode_eps=EPS, ode_solver_tol=TOL, noise=x1, device="cuda:0")
    dev, nfe_d, sec_d = tr.SDE.sample_model_ode(tr.score_fn, solver="device", **kw)
    info = dict(tr.SDE.last_ode)
    sci, nfe_s, sec_s = tr.SDE.sample_model_ode(tr.score_fn, solver="scipy", **kw)
    e = rel_mse(dev.cpu(), sci.cpu())
    print("ode production width B=4 T=32: device vs scipy %.3e; nfe %d / %d; %d accepted, %d rejected; seconds %.3f / %.3f (first calls)"
          % (e, nfe_d, nfe_s, info["accepted"], info["rejected"], sec_d, sec_s))
    assert info["route"] == "shared_t" and dev.shape == (B, T, z) and bool(torch.isfinite(dev).all()) and nfe_d >= 7
    assert e < 1e-3
