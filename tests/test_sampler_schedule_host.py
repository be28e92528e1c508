"""The sampling loop's host-side schedule (ldt_amd/diffusion.py), held on the CPU: which draw every update of the generic loop uses, how the
fused loop cuts a batch into sub-batches, and the folded predictor tables bit for bit.

`diffusion.ops` is replaced by a recording stand-in (in the manner of tests/test_block_routes_host.py): every entry point returns a tensor of
the shape the real one returns and the call's bound arguments are recorded, so `_sample_generic` runs on CPU tensors.  The expected tables
below were written by hand from the loop as it stood before it was split (one body, corrector chosen inside the inner loop): predictor step i
draws noise row / Philox stream k = i (1 + ncs), corrector step j of it draws k + 1 + j."""
import copy
import inspect

import numpy as np
import pytest
import torch

from ldt_amd import diffusion as D, ops as real_ops

N, B, SHAPE, SEED, OFF = 3, 2, (4, 4), 77, 5 * 16           # OFF: elem_offset of a rank whose first sample is global sample 5


class RecordingOps:
    """calls: [(name, {parameter: value})], every parameter bound by the real entry point's signature (defaults included)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError("%s: an entry point the stand-in does not know" % name[1:])
        result_of = getattr(self, "_" + name)
        sig = inspect.signature(getattr(real_ops, name))

        def recorded(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            self.calls.append((name, dict(bound.arguments)))
            return result_of(**bound.arguments)
        return recorded

    # x after step s of a run is a tensor filled with a fresh serial number, x_mean the negative of it: `denoise`, `record` and the dumps
    # can then be told apart by value
    def _sampler_step(self, x, x_mean_out, **kw):
        serial = float(len(self.calls))
        if x_mean_out is not None:
            x_mean_out.fill_(-serial)
        return torch.full_like(x, serial)

    def _philox_normal(self, shape, device, **kw):
        return torch.zeros(shape, device=device)

    def _batch_norm_sum(self, **kw):
        return None

    def _langevin_coef(self, **kw):
        return None


@pytest.fixture
def rec(monkeypatch):
    r = RecordingOps()
    monkeypatch.setattr(D, "ops", r)
    return r


@pytest.fixture
def sde(tiny_cfg):
    c = copy.deepcopy(tiny_cfg.sde)
    c.sample_N = N
    return D.DiffusionVPSDE(c)


def zeros_score_fn(t, x, label=None, condition=None):
    return torch.zeros_like(x), torch.zeros_like(x)


def run_generic(sde, batch=B, corrector=None, ncs=0, noise=None, seed=SEED, predictor="eulermaruyama", denoise=True, **extra):
    ts, coef, mode = sde.step_table(N, predictor, 1e-6)
    x = torch.zeros((batch,) + SHAPE)
    kw = dict(ts=ts, coef=coef, mode=mode, noise=noise, elem_offset=OFF, seed=seed, denoise=denoise, condition=None, label=None,
              trajectory=None, corrector=corrector, ncs=ncs, snr=0.01, global_batch=batch, n_valid=batch, sharded=False, print_steps=None,
              record=None)
    kw.update(extra)
    return sde._sample_generic(zeros_score_fn, x, **kw), mode


def draws(rec):
    """(name, step, mode, philox_mul, philox_add, elem_offset, seed) of every sampler_step / philox_normal call, in order.  (The Langevin
    update's own sampler_step takes its noise as an operand: it shows with the defaults step 0, mul 1, add 0, offset 0, seed 0.)"""
    out = []
    for name, a in rec.calls:
        if name == "sampler_step":
            out.append((name, a["step"], a["mode"], a["philox_mul"], a["philox_add"], a["elem_offset"], a["seed"]))
        elif name == "philox_normal":
            out.append((name, a["step"], None, None, None, a["elem_offset"], a["seed"]))
    return out


def noise_rows(rec, noise):
    """Which row of the injected `noise` each sampler_step was handed (by storage), in order."""
    rows = []
    for name, a in rec.calls:
        if name == "sampler_step":
            z = a["noise"]
            rows.append(None if z is None else (z.data_ptr() - noise.data_ptr()) // (z.element_size() * noise[0].numel()))
    return rows


def numbered_noise(rows, batch=B):
    return torch.arange(rows, dtype=torch.float32).view(-1, 1, 1, 1).expand((rows, batch) + SHAPE).contiguous()


# ---------------------------------------------------------------------------------------------------------------- the generic loop's draws
def test_no_corrector_one_draw_per_step(rec, sde):
    _, mode = run_generic(sde)
    assert mode == 1
    assert draws(rec) == [("sampler_step", 0, 1, 1, 0, OFF, SEED),
                          ("sampler_step", 1, 1, 1, 0, OFF, SEED),
                          ("sampler_step", 2, 1, 1, 0, OFF, SEED)]
    del rec.calls[:]
    noise = numbered_noise(N)
    run_generic(sde, noise=noise, seed=0, predictor="ancestral")
    assert noise_rows(rec, noise) == [0, 1, 2]
    assert [a["mode"] for _, a in rec.calls] == [0, 0, 0]                      # the ancestral predictor's own update form


def test_ancestral_corrector_two_steps(rec, sde):
    run_generic(sde, corrector="ancestral", ncs=2)
    S = "sampler_step"
    assert draws(rec) == [(S, 0, 1, 3, 0, OFF, SEED), (S, 0, 1, 3, 1, OFF, SEED), (S, 0, 1, 3, 2, OFF, SEED),
                          (S, 1, 1, 3, 0, OFF, SEED), (S, 1, 1, 3, 1, OFF, SEED), (S, 1, 1, 3, 2, OFF, SEED),
                          (S, 2, 1, 3, 0, OFF, SEED), (S, 2, 1, 3, 1, OFF, SEED), (S, 2, 1, 3, 2, OFF, SEED)]
    # the corrector's own folded table: [1, -2 snr^2 std, 2 snr std, 0] per step, handed to every corrector update
    ts = sde.step_table(N, "eulermaruyama", 1e-6)[0]
    std = sde.std(ts).double()
    want = torch.stack([torch.ones_like(std), -2.0 * 0.01 * 0.01 * std, 2.0 * 0.01 * std, torch.zeros_like(std)], 1).float()
    coefs = [a["coef"] for n, a in rec.calls if n == "sampler_step"]
    for k in (1, 2, 4, 5, 7, 8):
        assert torch.equal(coefs[k], want)
    del rec.calls[:]
    noise = numbered_noise(N * 3)
    run_generic(sde, corrector="ancestral", ncs=2, noise=noise, seed=0)
    assert noise_rows(rec, noise) == [0, 1, 2, 3, 4, 5, 6, 7, 8]


@pytest.mark.parametrize("batch", [1, SHAPE[0]])
def test_langevin_corrector_two_steps(rec, sde, batch):
    """B = 1 and B = tokens, the two batches the reference's broadcasting admits.  Each corrector step: a Philox draw of stream k + 1 + j, two
    norm sums over the valid rows, the step-size coefficients, and an update that takes the draw as its noise operand."""
    run_generic(sde, batch=batch, corrector="langevin", ncs=2)
    S, P = "sampler_step", "philox_normal"
    lv = (S, 0, 1, 1, 0, 0, 0)
    assert draws(rec) == [(S, 0, 1, 3, 0, OFF, SEED), (P, 1, None, None, None, OFF, SEED), lv, (P, 2, None, None, None, OFF, SEED), lv,
                          (S, 1, 1, 3, 0, OFF, SEED), (P, 4, None, None, None, OFF, SEED), lv, (P, 5, None, None, None, OFF, SEED), lv,
                          (S, 2, 1, 3, 0, OFF, SEED), (P, 7, None, None, None, OFF, SEED), lv, (P, 8, None, None, None, OFF, SEED), lv]
    names = [n for n, _ in rec.calls]
    assert names[:6] == [S, P, "batch_norm_sum", "batch_norm_sum", "langevin_coef", S]
    ts = sde.step_table(N, "eulermaruyama", 1e-6)[0]
    lc = [a for n, a in rec.calls if n == "langevin_coef"]
    assert [a["std_t"] for a in lc] == [float(sde.std(ts)[i]) for i in (0, 0, 1, 1, 2, 2)]
    assert all(a["n_total"] == batch and a["snr"] == 0.01 for a in lc)
    assert all(a["n_valid"] == batch and a["per_sample"] == 16 for n, a in rec.calls if n == "batch_norm_sum")
    philox_shapes = [tuple(a["shape"]) for n, a in rec.calls if n == P]
    assert philox_shapes == [(batch,) + SHAPE] * 6
    del rec.calls[:]
    noise = numbered_noise(N * 3, batch)
    run_generic(sde, batch=batch, corrector="langevin", ncs=2, noise=noise, seed=0)
    assert P not in [n for n, _ in rec.calls]                                  # injected noise replaces every draw
    assert noise_rows(rec, noise) == [0, 1, 2, 3, 4, 5, 6, 7, 8]


def test_record_trajectory_print_steps_and_denoise(rec, sde):
    record, trajectory = [], []
    out, _ = run_generic(sde, record=record, trajectory=trajectory)
    # serial numbers: sampler_step call s (1-based position in `calls`) returns x = s and writes x_mean = -s
    assert len(record) == N and all(len(r) == 4 for r in record)
    for i, (x_in, params, x_mean, x_new) in enumerate(record):
        assert float(x_in[0, 0, 0]) == float(i) and float(x_mean[0, 0, 0]) == -(i + 1.0) and float(x_new[0, 0, 0]) == i + 1.0
        assert tuple(params.shape) == (B,) + SHAPE
    assert len(trajectory) == 1 and tuple(trajectory[0].shape) == (N, B) + SHAPE
    assert [float(t[0, 0, 0]) for t in trajectory[0]] == [1.0, 2.0, 3.0]
    assert float(out[0, 0, 0]) == -3.0                                         # denoise=True: x_mean of the last step
    del rec.calls[:]
    out, _ = run_generic(sde, denoise=False)
    assert float(out[0, 0, 0]) == 3.0                                          # denoise=False: x

    # print_steps = 5 at N = 7: every = (7 - 1) // (5 - 2) = 2 -> x0, x_mean after steps 2, 4, 6, then the returned tensor
    n7 = 7
    ts, coef, mode = sde.step_table(n7, "eulermaruyama", 1e-6)
    for denoise, last in ((True, -7.0), (False, 7.0)):
        del rec.calls[:]
        kw = dict(ts=ts, coef=coef, mode=mode, noise=None, elem_offset=0, seed=SEED, denoise=denoise, condition=None, label=None,
                  trajectory=None, corrector=None, ncs=0, snr=0.01, global_batch=B, n_valid=B, sharded=False, print_steps=5, record=None)
        dump = sde._sample_generic(zeros_score_fn, torch.zeros((B,) + SHAPE), **kw)
        assert isinstance(dump, list) and [float(t[0, 0, 0]) for t in dump] == [0.0, -2.0, -4.0, -6.0, last]
    # N = 3: every = (3 - 1) // 3 = 0, the rule's own ZeroDivisionError at `(i + 1) % every`, kept
    with pytest.raises(ZeroDivisionError):
        run_generic(sde, print_steps=5)


# ---------------------------------------------------------------------------------------------------------------- the fused loop's partition
@pytest.mark.parametrize("batch,streams,bounds,cap", [
    (6, 1, [0, 6], 0),
    (6, 2, [0, 3, 6], 128),
    (6, 3, [0, 2, 4, 6], 85),
    (6, 4, [0, 1, 3, 4, 6], 64),
    (6, 8, [0, 1, 2, 3, 4, 5, 6], 42),                                         # clamped to B = 6 streams: 256 // 6
    (1, 2, [0, 1], 0),                                                         # clamped to one stream: the whole chip
])
def test_partition(batch, streams, bounds, cap):
    shape, off = (32, 4), 7 * 128
    parts = D.partition(batch, streams, int(np.prod(shape)), off)
    n = len(bounds) - 1
    assert n == max(1, min(streams, batch)) == len(parts)
    assert [p.lo for p in parts] == bounds[:-1] and [p.hi for p in parts] == bounds[1:]
    assert bounds == [batch * i // n for i in range(n + 1)]
    assert [p.slot for p in parts] == list(range(n))
    assert [p.gemm_wgs for p in parts] == [cap] * n
    assert [p.elem_offset for p in parts] == [off + lo * 128 for lo in bounds[:-1]]


# ---------------------------------------------------------------------------------------------------------------- step_table, bit for bit
def two_branch_step_table(sde, n, predictor, time_eps, probability_flow):
    """The reverse-diffusion and Euler-Maruyama tables as two branches with a signed dt, as they were written before the two were folded
    into one over |dt| (diffusion_continuous.py:141-150, :182-191); ancestral and ddim as they are."""
    ts = torch.linspace(1.0, time_eps, n)
    if predictor == "ancestral":
        idx = (ts * (n - 1) / 1.0).long()
        beta = sde.betas[idx]
        return ts, torch.stack([beta, sde.std(ts), torch.sqrt(1. - beta), torch.sqrt(beta)], 1).contiguous(), 0
    std = sde.std(ts).double()
    if predictor == "reversediffusion":
        dt = (1 - time_eps) / n
        g2 = sde.g2(ts).double(); ff = sde.f(ts).double()
        k = 0.5 if probability_flow else 1.0
        A = 1 - ff * dt
        Bc = -g2 * k * dt / std
        Cc = torch.zeros_like(g2) if probability_flow else torch.sqrt(g2) * np.sqrt(dt)
    elif predictor == "eulermaruyama":
        dt = -1.0 / n
        g2 = sde.g2(ts).double(); ff = sde.f(ts).double()
        k = 0.5 if probability_flow else 1.0
        A = 1 + ff * dt
        Bc = g2 * k * dt / std
        Cc = torch.zeros_like(g2) if probability_flow else torch.sqrt(g2) * np.sqrt(-dt)
    else:
        idx = (ts * (n - 1) / 1.0).long()
        at = sde.alphas_cump[idx].double()
        at_next = torch.where(idx - 1 < 0, torch.ones_like(at), sde.alphas_cump[(idx - 1).clamp_min(0)].double())
        A = at_next.sqrt() / at.sqrt()
        Bc = -at_next.sqrt() * (1 - at).sqrt() / at.sqrt() + (1 - at_next).sqrt()
        Cc = torch.zeros_like(at)
    return ts, torch.stack([A, Bc, Cc, torch.zeros_like(A)], 1).float().contiguous(), 1


FAMILIES = {"vpsde": {}, "sub_vpsde": {}, "vesde": dict(sigma2_min=0.01, sigma2_max=4.0, sigma2_0=0.01),
            "geometric_sde": dict(sigma2_min=3e-5, sigma2_max=0.999, sigma2_0=0.0)}


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("n", [25, 1000])
def test_step_table_equals_the_two_branch_form(tiny_cfg, family, n):
    c = copy.deepcopy(tiny_cfg.sde)
    c.sde_type, c.sample_N = family, n
    for k, v in FAMILIES[family].items():
        setattr(c, k, v)
    sde = D.make_diffusion(c)
    compared = 0
    for predictor in D.PREDICTORS:
        if predictor in ("ancestral", "ddim") and family != "vpsde":          # no betas table outside the VP-SDE, as upstream
            with pytest.raises(AttributeError):
                sde.step_table(n, predictor, 1e-6)
            continue
        for pf in (False, True):
            for eps in (1e-6, 1e-2):
                ts, coef, mode = sde.step_table(n, predictor, eps, pf)
                wts, wcoef, wmode = two_branch_step_table(sde, n, predictor, eps, pf)
                assert mode == wmode and torch.equal(ts, wts), (predictor, pf, eps)
                assert coef.dtype == torch.float32 and coef.is_contiguous() and torch.equal(coef, wcoef), (predictor, pf, eps)
                compared += 1
    assert compared == (16 if family == "vpsde" else 8)
