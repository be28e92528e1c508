"""GPU (-m gpu): the loss kernels evaluation reports from, on the paths test_gpu_eval.py and test_gpu_hybrid.py do not sweep
(csrc/eval_loss.hip, csrc/nelbo_terms.hip).  References are float64 (or, where the kernel promises the bits, the fp32 expression) on the
kernels' own fp32 inputs and outputs; every case is a few MB.

  * ldt_diffuse_q past its 2048 x 256 cap: the grid-stride loop takes a second and a third pass, and sample boundaries (per-sample m, var)
    fall inside each; injected noise and the Philox form, bit for bit.
  * ldt_dsm_loss / ldt_nelbo_terms with B > 1024: the second stage's lanes take two samples; vector (per_sample 8) and scalar (7) forms,
    per-sample weights from 0.05 to 30.
  * the scalar fallback chosen by misalignment (views one float into their storage) where the sizes would allow 16-byte accesses.
  * ldt_reparam_kl's log q(z) and KL per element, at a bound derived from the kernel's operation order (kernel_checks.reparam_kl_ref)."""
import collections

import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

RATIOS = collections.defaultdict(float)
N_OVER = 2 * (2048 * 256 * 4) + 4 * 259           # floats: crosses the 2048-block cap of ldt_diffuse_q twice, tail of 259 vectors
PER_SAMPLE = 20                                   # divides N_OVER, a multiple of 4: 209,767 samples of 5 vectors
LO, HI = -30.0, 10.0


def sqrt_rn(v):
    """The correctly rounded fp32 square root (test_gpu_eval.py)."""
    return torch.sqrt(v.double()).float()


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


def dsm_reference(eta, params, weight, l1):
    """Latent_SDE_Trainer.py:83-87 in float64: (mean over everything, per-sample means)."""
    d = eta.double() - params.double()
    dist = (d.abs() if l1 else d * d) * weight.double()[:, None]
    return dist.mean(), dist.mean(1)


def off_by_one(t):
    """A copy of t that is a contiguous view one float into its storage: 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def first_difference(got, want, per_sample):
    bad = torch.nonzero(got.reshape(-1) != want.reshape(-1)).flatten()
    if bad.numel() == 0:
        return None
    i = int(bad[0])
    return "%d of %d elements differ, first at element %d (vector %d = sweep %d + %d, sample %d)" % (
        bad.numel(), got.numel(), i, i // 4, (i // 4) // (2048 * 256), (i // 4) % (2048 * 256), i // per_sample)


def test_diffuse_q_past_the_grid_cap():
    from ldt_amd import ops
    assert N_OVER % PER_SAMPLE == 0 and PER_SAMPLE % 4 == 0 and (2048 * 256 * 4) % PER_SAMPLE != 0
    B = N_OVER // PER_SAMPLE
    g = torch.Generator().manual_seed(23)
    x0, eta = torch.randn(B, PER_SAMPLE, generator=g) * 3.0, torch.randn(B, PER_SAMPLE, generator=g)
    odd = (torch.arange(B) % 2).float()                                                     # neighbours differ: a wrong b = 4 i / per_sample shows
    m, var = torch.rand(B, generator=g) * 0.4 + 0.5 * odd, torch.rand(B, generator=g) * 0.4 + 0.5 * (1 - odd) + 1e-7
    assert bool((m[1:] != m[:-1]).all()) and bool((var[1:] != var[:-1]).all())
    expr = lambda e: x0 * m[:, None] + sqrt_rn(var)[:, None] * e                            # torch-CPU fp32, the reference's expression
    xd, md, vd = x0.cuda(), m.cuda(), var.cuda()
    xt, eta_back = ops.diffuse_q(xd, md, vd, eta.cuda())
    assert first_difference(xt.cpu(), expr(eta), PER_SAMPLE) is None, first_difference(xt.cpu(), expr(eta), PER_SAMPLE)
    assert torch.equal(eta_back.cpu(), eta)
    # (every element is compared, so the windows of kernel_checks.sweep_windows and both sides of every sample boundary are among them)
    # the Philox form: the stream of ldt_philox_normal, and the result of injecting it
    seed, step = 0x0123456789ABCDEF % (2 ** 62), 3
    xt_p, eta_p = ops.diffuse_q(xd, md, vd, None, seed=seed, step=step)
    want_eta = ops.philox_normal((B, PER_SAMPLE), "cuda", seed, step=step)
    assert first_difference(eta_p.cpu(), want_eta.cpu(), PER_SAMPLE) is None, first_difference(eta_p.cpu(), want_eta.cpu(), PER_SAMPLE)
    assert first_difference(xt_p.cpu(), expr(eta_p.cpu()), PER_SAMPLE) is None, first_difference(xt_p.cpu(), expr(eta_p.cpu()), PER_SAMPLE)
    ref, tol = kc.philox_normal_ref(seed, step, 2048 * 256 - 8, 16)                          # across the first sweep boundary, against numpy
    kc.assert_elementwise(eta_p.reshape(-1, 4)[2048 * 256 - 8: 2048 * 256 + 8].cpu(), ref, tol, "diffuse_q Philox at the sweep boundary")


def loss_inputs(B, per_sample, seed):
    g = torch.Generator().manual_seed(seed)
    eta, params = torch.randn(B, per_sample, generator=g), torch.randn(B, per_sample, generator=g) * 0.7
    logqz = -0.9189385332 - 0.5 * (torch.randn(B, per_sample, generator=g) * 1.5 - 1.0) - 0.5 * torch.randn(B, per_sample, generator=g) ** 2
    w = 0.05 * (600.0 ** torch.rand(B, generator=g))                                       # 0.05 .. 30, a neighbour's weight is far off
    return eta, params, logqz, w


def nelbo_reference(eta, params, logqz, w):
    dist = (eta.double() - params.double()) ** 2 * w.double()[:, None]
    return torch.stack([dist.sum(1), logqz.double().sum(1)], 1)


@pytest.mark.parametrize("per_sample", [8, 7])
@pytest.mark.parametrize("l1", [False, True])
def test_dsm_loss_second_stage_past_1024_samples(per_sample, l1):
    from ldt_amd import ops
    B = 1025 + 64
    eta, params, _, w = loss_inputs(B, per_sample, 31 + per_sample)
    mean, per = ops.dsm_loss(eta.cuda(), params.cuda(), w.cuda(), l1=l1)
    mean64, per64 = dsm_reference(eta, params, w, l1)
    print("dsm_loss B %d per_sample %d l1=%d: relerr per sample %.2e, batch %.2e" % (B, per_sample, l1, relerr(per, per64), relerr(mean, mean64)))
    assert per.shape == (B,) and relerr(per, per64) <= 1e-6 and relerr(mean, mean64) <= 1e-6
    shifted = dsm_reference(eta, params, torch.roll(w, 1), l1)[1]                           # a sample read with its neighbour's weight fails
    assert float(((shifted - per64).abs() / per64).min()) > 1e-5                            # ten times the bound, at the least


@pytest.mark.parametrize("per_sample", [8, 7])
def test_nelbo_terms_second_stage_past_1024_samples(per_sample):
    from ldt_amd import ops
    B = 1025 + 64
    eta, params, logqz, w = loss_inputs(B, per_sample, 41 + per_sample)
    tot, per = ops.nelbo_terms(eta.cuda(), params.cuda(), logqz.cuda(), w.cuda())
    want = nelbo_reference(eta, params, logqz, w)
    print("nelbo_terms B %d per_sample %d: relerr per sample %.2e, batch %.2e" % (B, per_sample, relerr(per, want), relerr(tot, want.sum(0))))
    assert per.shape == (B, 2) and relerr(per, want) <= 1e-6 and relerr(tot, want.sum(0)) <= 1e-6


def test_misaligned_inputs_take_the_scalar_form():
    from ldt_amd import ops
    # reparam_kl: z a multiple of 4, each input / the output in turn one float into its storage
    rows, z, T = 48, 8, 4
    g = torch.Generator().manual_seed(5)
    post = torch.randn(rows, 2 * z, generator=g); post[:, z:] = post[:, z:] * 1.5 - 1.0
    post[0, z], post[1, z] = 50.0, -50.0
    noise = torch.randn(rows, z, generator=g)
    post, noise = post.cuda(), noise.cuda()
    run = lambda p, nz, o: (o,) + ops.reparam_kl(p, nz, o, LO, HI, T, want_stats=True)
    aligned = run(post, noise, torch.zeros(rows, z, device="cuda"))
    for which in range(3):
        got = run(off_by_one(post) if which == 0 else post, off_by_one(noise) if which == 1 else noise,
                  off_by_one(torch.zeros(rows, z, device="cuda")) if which == 2 else torch.zeros(rows, z, device="cuda"))
        for name, a, b in zip(("out", "mu", "logvar", "kl", "logqz"), aligned, got):
            assert torch.equal(a, b), "reparam_kl misaligned argument %d: %s differs" % (which, name)
        assert relerr(got[5], aligned[5]) <= 1e-6                                           # the sample sums: another order of the same terms
    # dsm_loss / nelbo_terms: per_sample a multiple of 4
    B, per_sample = 37, 24
    eta, params, logqz, w = loss_inputs(B, per_sample, 7)
    ed, pd, qd, wd = eta.cuda(), params.cuda(), logqz.cuda(), w.cuda()
    mean64, per64 = dsm_reference(eta, params, w, False)
    want = nelbo_reference(eta, params, logqz, w)
    for which in range(3):
        e, p, q = (off_by_one(t) if which == i else t for i, t in enumerate((ed, pd, qd)))
        if which < 2:
            mean, per = ops.dsm_loss(e, p, wd)
            assert relerr(per, per64) <= 1e-6 and relerr(mean, mean64) <= 1e-6, which
        tot, per2 = ops.nelbo_terms(e, p, q, wd)
        assert relerr(per2, want) <= 1e-6 and relerr(tot, want.sum(0)) <= 1e-6, which


def reparam_kl_case(B, T, z, edge_row):
    g = torch.Generator().manual_seed(B * 1000 + z)
    rows = B * T
    post = torch.randn(rows, 2 * z, generator=g)
    post[:, z:] = post[:, z:] * 1.5 - 1.0
    post[0, z] = 50.0; post[1, z] = -50.0                       # both clamps
    noise = torch.randn(rows, z, generator=g)
    if edge_row:                                                # a row with logvar at both clamps and noise of magnitude 6
        post[rows - 1, z:] = torch.where(torch.arange(z) % 2 == 0, torch.tensor(50.0), torch.tensor(-50.0))
        noise[rows - 1] = torch.where(torch.arange(z) % 4 < 2, torch.tensor(6.0), torch.tensor(-6.0))
    return post.cuda(), noise.cuda()


@pytest.mark.parametrize("B,T,z,edge_row", [(64, 256, 20, False), (3, 7, 5, False), (4, 8, 40, False), (4, 8, 40, True)])
def test_reparam_kl_per_element(B, T, z, edge_row):
    from ldt_amd import ops
    post, noise = reparam_kl_case(B, T, z, edge_row)
    eps = torch.zeros(B * T, z, device="cuda")
    mu, lv, kl, lq, ks = ops.reparam_kl(post, noise, eps, LO, HI, T, want_stats=True)
    if edge_row:
        assert float(lv[-1].max()) == HI and float(lv[-1].min()) == LO and float(eps[-1].abs().max()) > 100.0
    lq64, tol_q, kl64, tol_k = kc.reparam_kl_ref(eps.cpu(), mu.cpu(), lv.cpu())
    what = "reparam_kl B %d T %d z %d%s" % (B, T, z, " + edge row" if edge_row else "")
    rq = kc.assert_elementwise(lq.cpu(), lq64, tol_q, what + " logqz")
    rk = kc.assert_elementwise(kl.cpu(), kl64, tol_k, what + " kl")
    print("%s: max err / tol logqz %.3f, kl %.3f" % (what, rq, rk))
    RATIOS["reparam_kl logqz"] = max(RATIOS["reparam_kl logqz"], rq)
    RATIOS["reparam_kl kl"] = max(RATIOS["reparam_kl kl"], rk)


def test_zz_margins():
    for k in sorted(RATIOS):
        print("worst err / tol, %-20s %.3f" % (k + ":", RATIOS[k]))
    assert all(v <= 1.0 for v in RATIOS.values())
