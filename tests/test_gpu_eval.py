"""GPU (-m gpu): held-out evaluation on the HIP path — the three loss kernels (ldt_reparam_kl, ldt_diffuse_q, ldt_dsm_loss),
`Compressor.forward(want_kl=True)`, `Trainer.val_loss`, `CompressorTrainer` / `CompletionCompressorTrainer`.

Yardsticks: tests/golden/eval_tiny.npz (the reference's own numbers; tests/test_eval_host.py pins the fp32 restatement used
here against it), fp64 evaluations of the formulas on the kernels' own fp32 inputs, and bit-equality where the library
promises it (ldt_reparam_kl vs ldt_reparam, injected-noise ldt_diffuse_q vs the torch-CPU fp32 expression with a correctly rounded
square root, in-kernel Philox vs ldt_philox_normal, run-to-run)."""
import copy
import os

import numpy as np
import pytest
import torch

import kernel_checks as kc
from conftest import GOLDEN, load_golden, rel_mse

pytestmark = pytest.mark.gpu


def eval_golden():
    z = np.load(os.path.join(GOLDEN, "eval_tiny.npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def dsm_reference(eta, params, weight, l1):
    """Latent_SDE_Trainer.py:83-87 in fp64: (mean over everything, per-sample means)."""
    d = eta.double() - params.double()
    dist = d.abs() if l1 else d * d
    if weight is not None:
        dist = dist * weight.double().view(-1, *([1] * (dist.dim() - 1)))
    return dist.mean(), dist.reshape(dist.shape[0], -1).mean(1)


def sqrt_rn(v):
    """The correctly rounded fp32 square root (an fp64 root rounded once more).  torch's vectorised CPU `sqrt` is not: it is up to one ulp
    off for a share of the inputs that depends on the host's instruction set, so "bit-equal to torch-CPU" can only mean this."""
    return torch.sqrt(v.double()).float()


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("B,T,z,L", [(64, 256, 20, 6), (3, 7, 5, 2), (4, 8, 40, 3)])
def test_reparam_kl_kernel(B, T, z, L):
    """(64, 256, 20, 6): the production encode's posterior draw, 16-byte accesses into a strided slice of all_eps (ldo = L z > z);
    (3, 7, 5, 2): rows_per_sample x z = 35, not a multiple of 4 — the scalar form; (4, 8, 40, 3): the tiny fixture's shape."""
    from ldt_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + z)
    rows = B * T
    post = torch.randn(rows, 2 * z, generator=g)
    post[:, z:] = post[:, z:] * 1.5 - 1.0
    post[0, z] = 50.0; post[1, z] = -50.0                       # both clamps
    noise = torch.randn(rows, z, generator=g)
    post, noise = post.cuda(), noise.cuda()
    lo, hi = -30.0, 10.0
    plain = torch.zeros(rows, L * z, device="cuda")
    fused = torch.zeros(rows, L * z, device="cuda")
    j = L - 1
    mu0, lv0 = ops.reparam(post, noise, plain[:, z * j: z * (j + 1)], lo, hi, want_stats=True)
    mu, lv, kl, lq, ks = ops.reparam_kl(post, noise, fused[:, z * j: z * (j + 1)], lo, hi, T, want_stats=True)
    assert torch.equal(fused, plain) and torch.equal(mu, mu0) and torch.equal(lv, lv0)      # bit-identical to ldt_reparam
    assert float(fused[:, :z * j].abs().max()) == 0.0                                       # nothing outside the slice is written
    assert float(lv.max()) == hi and float(lv.min()) >= lo
    eps = fused[:, z * j: z * (j + 1)]
    lq64, tol_q, kl64, tol_k = kc.reparam_kl_ref(eps.cpu(), mu.cpu(), lv.cpu())              # per element, from the kernel's operation order
    kc.assert_elementwise(lq.cpu(), lq64, tol_q, "reparam_kl logqz")
    kc.assert_elementwise(kl.cpu(), kl64, tol_k, "reparam_kl kl")
    assert ks.shape == (B,)
    assert relerr(ks, kl.double().view(B, -1).sum(1)) <= 1e-6                               # the fixed-order sum of the kernel's own kl
    assert relerr(ks, kl64.view(B, -1).sum(1)) <= 1e-5
    # without the statistics and a second time: the same bits
    again = torch.zeros_like(fused)
    mu2, lv2, kl2, lq2, ks2 = ops.reparam_kl(post, noise, again[:, z * j: z * (j + 1)], lo, hi, T)
    assert mu2 is None and lv2 is None
    assert torch.equal(again, fused) and torch.equal(kl2, kl) and torch.equal(lq2, lq) and torch.equal(ks2, ks)


def test_reparam_kl_null_outputs_and_errors():
    from ldt_amd import _lib, ops
    lib = _lib.lib()
    rows, z, T = 16, 8, 4
    post, noise = torch.randn(rows, 2 * z).cuda(), torch.randn(rows, z).cuda()
    out, ref = torch.empty(rows, z, device="cuda"), torch.empty(rows, z, device="cuda")
    ops.reparam(post, noise, ref, -30., 10.)
    rc = lib.ldt_reparam_kl(post.data_ptr(), noise.data_ptr(), out.data_ptr(), z, None, None, None, None, None, rows, T, z, -30., 10.,
                            ops.stream_ptr())
    assert rc == 0 and torch.equal(out, ref)                     # every optional output null: ldt_reparam
    rc = lib.ldt_reparam_kl(post.data_ptr(), noise.data_ptr(), out.data_ptr(), z - 1, None, None, None, None, None, rows, T, z, -30., 10.,
                            ops.stream_ptr())
    assert rc == -2                                              # ldo < z
    with pytest.raises(_lib.LdtHipError):
        ops.reparam_kl(post, noise, out, -30., 10., 5)           # 16 rows are not a whole number of 5-row samples


def test_diffuse_q_kernel():
    from ldt_amd import ops
    g = torch.Generator().manual_seed(5)
    B, T, z = 64, 256, 120
    x0, eta = torch.randn(B, T, z, generator=g) * 3.0, torch.randn(B, T, z, generator=g)
    m, var = torch.rand(B, generator=g), torch.rand(B, generator=g) * 0.999 + 1e-7
    want = x0 * m[:, None, None] + sqrt_rn(var)[:, None, None] * eta                        # torch-CPU fp32, the reference's expression
    xt, eta_back = ops.diffuse_q(x0.cuda(), m.cuda(), var.cuda(), eta.cuda())
    assert torch.equal(xt.cpu(), want) and torch.equal(eta_back.cpu(), eta)
    # in-kernel Philox: the stream of ldt_philox_normal(seed, step, elem_offset = 0), bit for bit; and the result of injecting it
    seed, step = 0x1234567890ABCDEF % (2 ** 62), 7
    xt_p, eta_p = ops.diffuse_q(x0.cuda(), m.cuda(), var.cuda(), None, seed=seed, step=step)
    assert torch.equal(eta_p, ops.philox_normal((B, T, z), "cuda", seed, step=step))
    assert torch.equal(xt_p, ops.diffuse_q(x0.cuda(), m.cuda(), var.cuda(), eta_p)[0])
    assert torch.equal(xt_p.cpu(), x0 * m[:, None, None] + sqrt_rn(var)[:, None, None] * eta_p.cpu())
    assert abs(float(eta_p.mean())) < 5e-3 and abs(float(eta_p.std()) - 1.0) < 5e-3
    # a sharded batch reproduces its rows by offset: rows [16, 32) of the stream
    per = T * z
    assert torch.equal(eta_p[16:32], ops.philox_normal((16, T, z), "cuda", seed, step=step, elem_offset=16 * per))
    assert not torch.equal(eta_p, ops.diffuse_q(x0.cuda(), m.cuda(), var.cuda(), None, seed=seed, step=step + 1)[1])
    # DiffusionBase.sample_q routes device latents with per-sample scalars here
    import ldt_amd
    sde = ldt_amd.DiffusionVPSDE(ldt_amd.airplane_config().sde)
    xq = sde.sample_q(x0.cuda(), eta.cuda(), var.cuda()[:, None, None], m.cuda()[:, None, None])
    assert torch.equal(xq.cpu(), want)


@pytest.mark.parametrize("shape", [(64, 256, 120), (5, 7, 11)])
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
def test_dsm_loss_kernel(shape, l1, weighted):
    """(64, 256, 120): B x per_sample of the headline shape; (5, 7, 11): per_sample = 77, the ragged (scalar) form."""
    from ldt_amd import ops
    g = torch.Generator().manual_seed(11)
    eta, params = torch.randn(shape, generator=g), torch.randn(shape, generator=g) * 0.7
    w = (torch.rand(shape[0], generator=g) + 0.5) if weighted else None
    mean, per = ops.dsm_loss(eta.cuda(), params.cuda(), None if w is None else w.cuda(), l1=l1)
    mean64, per64 = dsm_reference(eta, params, w, l1)
    assert mean.shape == () and per.shape == (shape[0],) and mean.is_cuda
    assert relerr(per, per64) <= 1e-6 and relerr(mean, mean64) <= 1e-6
    mean2, per2 = ops.dsm_loss(eta.cuda(), params.cuda(), None if w is None else w.cuda(), l1=l1)
    assert torch.equal(mean2, mean) and torch.equal(per2, per)                              # fixed summation order


# ------------------------------------------------------------------------------------------------ tiny fixture
@pytest.fixture(scope="module")
def env(tiny_cfg):
    import ldt_amd
    assert torch.cuda.is_available()
    _, ssd = load_golden("score_tiny")
    _, csd = load_golden("trainer_sample_tiny")
    fwd, _ = load_golden("compressor_fwd_tiny")
    score = ldt_amd.Score(tiny_cfg.score)
    score.load_state_dict(ssd["w"], strict=True)
    comp = ldt_amd.Compressor(tiny_cfg.compressor)
    comp.load_state_dict(csd["c"], strict=True)
    tr = ldt_amd.Trainer(tiny_cfg, score, comp, "cuda:0")
    return dict(ldt=ldt_amd, cfg=tiny_cfg, tr=tr, comp=tr.compressor, score=tr.model, csd=csd["c"], fwd=fwd, g=eval_golden())


def test_compressor_forward_want_kl_golden(env):
    comp, fwd, g = env["comp"], env["fwd"], env["g"]
    pts, noise = fwd["pts"].cuda(), list(fwd["post_noise"])
    off = comp(pts, post_noise=noise)
    on = comp(pts, post_noise=noise, want_kl=True)
    assert off["kls"] is None and off["all_logqz"] is None and "kl_sample_sum" not in off
    assert torch.equal(on["all_eps"], off["all_eps"]) and torch.equal(on["set"], off["set"])          # the draw itself is unchanged
    B, T, z, L = pts.shape[0], comp.z_scales, comp.z_dim, comp.n_layers
    assert len(on["kls"]) == L and len(on["all_logqz"]) == L
    for j in range(L):
        assert on["kls"][j].shape == (B, z, T) and on["all_logqz"][j].shape == (B, z, T)             # channels-first, as upstream
        assert rel_mse(on["kls"][j].transpose(1, 2).cpu(), g["kls"][j]) <= 1e-4
        assert rel_mse(on["all_logqz"][j].transpose(1, 2).cpu(), g["all_logqz"][j]) <= 1e-4
    # the expressions the reference trainers write on them
    kl_cat = torch.cat(on["kls"], dim=1)
    assert kl_cat.shape == (B, L * z, T)
    assert torch.cat(on["all_logqz"], dim=1).transpose(1, 2).shape == (B, T, L * z)
    kl_rms = float(g["kls"].double().pow(2).mean().sqrt())
    print("want_kl vs reference: rel-MSE kls %.3e, all_logqz %.3e; mean KL %.6f vs %.6f" % (
        rel_mse(kl_cat.cpu(), torch.cat([k.transpose(1, 2) for k in g["kls"]], 1)),
        rel_mse(torch.cat(on["all_logqz"], 1).cpu(), torch.cat([k.transpose(1, 2) for k in g["all_logqz"]], 1)),
        float(kl_cat.mean()), float(g["kl_loss"])))
    # the KL terms change sign from element to element (mean 0.04, rms 0.29): a rel-MSE of 1e-4 bounds the mean to 1e-2 rms
    assert abs(float(kl_cat.mean()) - float(g["kl_loss"])) <= 1e-2 * kl_rms
    assert on["kl_sample_sum"].shape == (B, L)
    assert relerr(on["kl_sample_sum"], torch.stack([k.double().reshape(B, -1).sum(1) for k in on["kls"]], 1)) <= 1e-6
    # with the posterior statistics as well
    st = comp(pts, post_noise=noise, want_kl=True, want_stats=True)
    assert torch.equal(st["all_eps"], off["all_eps"]) and st["posteriors"][0][1].shape == (B, T, z)
    assert torch.equal(st["kls"][0], on["kls"][0])


def _val_data(env):
    return {"te_points": env["fwd"]["pts"], "cate_idx": torch.zeros(env["fwd"]["pts"].shape[0], dtype=torch.long)}


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
def test_val_loss_golden(env, monkeypatch, loss_type):
    """Injected t_index / eta and the recorded posterior noise: the reference's loss (eval_tiny.npz), both cfg.opt.loss_type branches."""
    tr, g, fwd = env["tr"], env["g"], env["fwd"]
    cfg = copy.deepcopy(env["cfg"])
    cfg.opt.loss_type = loss_type
    monkeypatch.setattr(tr, "cfg", cfg)
    noise = list(fwd["post_noise"])
    real_forward = tr.compressor.forward
    monkeypatch.setattr(tr.compressor, "forward", lambda x, *a, **k: real_forward(x, *a, post_noise=noise, **k))
    loss = tr.val_loss(_val_data(env), t_index=g["val/idx"], eta=g["val/eta"])
    assert loss.shape == () and loss.is_cuda
    want = float(g["val/loss_" + loss_type])
    print("val_loss %s: %.7f vs the reference's %.7f (relative %.2e)" % (loss_type, float(loss), want, abs(float(loss) - want) / want))
    # the loss goes through the bf16 Score forward (params held to a rel-MSE of 1e-4, measured ~1e-6 = 1e-3 rms): measured 1.3e-4 (l2), below 1e-4 (l1)
    assert abs(float(loss) - want) <= 1e-3 * want
    last = tr.last_val_loss
    assert torch.equal(last["t"].cpu(), g["val/t"])
    assert rel_mse(last["xt"].cpu(), g["val/xt"]) <= 1e-4 and rel_mse(last["params"].cpu(), g["val/params"]) <= 1e-4


def test_val_loss_ema_swap_seeding_and_rng_consumption(env):
    ldt, cfg = env["ldt"], env["cfg"]
    _, ssd = load_golden("score_tiny")
    score = ldt.Score(cfg.score)
    score.load_state_dict(ssd["w"], strict=True)
    comp = ldt.Compressor(cfg.compressor)
    comp.load_state_dict(env["csd"], strict=True)
    tr = ldt.Trainer(cfg, score, comp, "cuda:0")
    data = _val_data(env)
    idx = env["g"]["val/idx"]

    def run(**kw):
        torch.manual_seed(3)                                     # keys the Compressor's posterior noise (and eta when no seed is given)
        return tr.val_loss(data, **kw)

    base = run(t_index=idx, seed=77)
    assert torch.equal(run(t_index=idx, seed=77), base)          # same seed: the same loss, bit for bit
    assert not torch.equal(run(t_index=idx, seed=78), base)
    # EMA weights are what is evaluated, and the model's own weights are back afterwards — also when the forward raises
    before = [p.data.clone() for p in tr.model.parameters()]
    for p in tr.model.parameters():
        tr.optimizer.state[p] = {"ema": p.data * 0.5}
    ema_loss = run(t_index=idx, seed=77)
    assert not torch.equal(ema_loss, base)
    assert all(torch.equal(p.data, b) for p, b in zip(tr.model.parameters(), before))
    assert all(torch.equal(tr.optimizer.state[p]["ema"], b * 0.5) for p, b in zip(tr.model.parameters(), before))
    with pytest.raises(ValueError):
        run(t_index=idx[:1], seed=77)                            # one index for a batch of two
    assert all(torch.equal(p.data, b) for p, b in zip(tr.model.parameters(), before))
    tr.optimizer.state.clear()
    # default path: exactly one np.random.choice(arange(train_N), B) on numpy's global generator, and its times are used
    np.random.seed(2024)
    want_idx = np.random.choice(np.arange(cfg.sde.train_N), 2, replace=True)
    after = np.random.get_state()
    np.random.seed(2024)
    default = run()
    got = np.random.get_state()
    assert got[0] == after[0] and np.array_equal(got[1], after[1]) and got[2:] == after[2:]
    want_t = torch.linspace(1.0, cfg.sde.sample_time_eps, cfg.sde.train_N)[torch.from_numpy(want_idx)]
    assert torch.equal(tr.last_val_loss["t"].cpu(), want_t) and bool(torch.isfinite(default))
    # the label path (cfg.data.num_categorys > 1 reads data['cate_idx']) on a label-conditional Score
    c2 = copy.deepcopy(cfg)
    c2.data.num_categorys, c2.score.num_categorys = 3, 3
    torch.manual_seed(0)
    tr2 = ldt.Trainer(c2, ldt.Score(c2.score), comp, "cuda:0")
    d0, d1 = dict(data), dict(data)
    d1["cate_idx"] = torch.ones(2, dtype=torch.long)
    torch.manual_seed(3); l0 = tr2.val_loss(d0, t_index=idx, seed=5)
    torch.manual_seed(3); l1 = tr2.val_loss(d1, t_index=idx, seed=5)
    assert bool(torch.isfinite(l0)) and not torch.equal(l0, l1)


# ------------------------------------------------------------------------------------------------ Compressor trainers
def _loader(n_batches, B, N, cates=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n_batches):
        pts = torch.randn(B, N, 3, generator=g) * 0.4
        d = {"te_points": pts, "tr_points": torch.randn(B, N, 3, generator=g) * 0.4,
             "shift": torch.randn(B, 1, 3, generator=g), "scale": torch.rand(B, 1, 1, generator=g) + 0.5,
             "cate_idx": torch.zeros(B, dtype=torch.long) if cates is None else cates[i]}
        out.append(d)
    return out


@pytest.mark.parametrize("multi", [False, True])
def test_compressor_trainer_reconstrustion(env, tmp_path, multi):
    ldt = env["ldt"]
    from ldt_amd.metrics import compute_all_metrics
    cfg = copy.deepcopy(env["cfg"])
    cfg.log.save_path = str(tmp_path)
    B, N = 4, 64
    cates = None
    if multi:
        cfg.data.num_categorys, cfg.data.test_batch_size = 3, 5
        cates = [torch.tensor([2, 0, 2, 1]), torch.tensor([2, 2, 2, 2]), torch.tensor([0, 1, 2, 0])]
    loader = _loader(3, B, N, cates)
    comp = ldt.Compressor(cfg.compressor)
    comp.load_state_dict(env["csd"], strict=True)
    tr = ldt.CompressorTrainer(cfg, comp, "cuda:0")
    torch.manual_seed(9)
    res = tr.reconstrustion(loader, val_cate=2) if multi else tr.reconstrustion(loader)
    # by hand, on the same CPU-generator draws (one per Compressor.forward call, in the same order)
    torch.manual_seed(9)
    if not multi:
        rec = torch.cat([comp(d["te_points"].cuda())["set"] * d["scale"].cuda() + d["shift"].cuda() for d in loader], 0)
        ref = torch.cat([d["te_points"].cuda() * d["scale"].cuda() + d["shift"].cuda() for d in loader], 0)
    else:
        keep = [d["cate_idx"] == 2 for d in loader]
        pts = torch.cat([d["te_points"][k] for d, k in zip(loader, keep)], 0).cuda()
        sh = torch.cat([d["shift"][k] for d, k in zip(loader, keep)], 0).cuda()
        sc = torch.cat([d["scale"][k] for d, k in zip(loader, keep)], 0).cuda()
        assert pts.shape[0] == 7                                 # two batches of test_batch_size = 5: 5 + 2
        lab = lambda n: torch.full((n,), 2, dtype=torch.int32, device="cuda")
        rec = torch.cat([comp(pts[:5], label=lab(5))["set"], comp(pts[5:], label=lab(2))["set"]], 0) * sc + sh
        ref = pts * sc + sh
    want = compute_all_metrics(rec, ref, batch_size=128)
    assert set(res) == {"val/gen/%s" % k for k in want}
    for k, v in want.items():
        assert res["val/gen/%s" % k] == (v if isinstance(v, float) else v.item()), k
    dumped = np.load(os.path.join(str(tmp_path), "rec_ep1.npy"))
    assert np.array_equal(dumped, rec.cpu().numpy())             # the de-normalised reconstructions


def test_compressor_trainer_sample_valsample_resume_eval_losses(env, tmp_path):
    ldt = env["ldt"]
    cfg = copy.deepcopy(env["cfg"])
    cfg.log.save_path = str(tmp_path)
    comp = ldt.Compressor(cfg.compressor)
    comp.load_state_dict(env["csd"], strict=True)
    tr = ldt.CompressorTrainer(cfg, comp, "cuda:0")
    # sample: Compressor.sample on given latents
    a, _ = load_golden("decoder_tiny")
    assert rel_mse(tr.sample(2, 64, given_eps=a["given_eps"].cuda()).cpu(), a["points"]) < 1e-4
    # valsample: prior samples for every test shape, the dump and the metric keys
    loader = _loader(2, 3, 64)
    res = tr.valsample(loader, 64)
    assert np.load(os.path.join(str(tmp_path), "smp_ep1.npy")).shape == (6, 64, 3)
    assert "val/gen/1-NN-CD-acc" in res and all(isinstance(v, float) for v in res.values())
    # eval_losses vs the restatement on the forward's own outputs
    fwd = env["fwd"]
    noise = list(fwd["post_noise"])
    real_forward = comp.forward
    comp.forward = lambda x, *a_, **k: real_forward(x, *a_, post_noise=noise, **k)
    try:
        losses = tr.eval_losses(fwd["pts"])
        out = comp(fwd["pts"].cuda(), want_kl=True)
    finally:
        del comp.forward
    kl_rms = float(env["g"]["kls"].double().pow(2).mean().sqrt())
    assert abs(float(losses["kl_loss"]) - float(env["g"]["kl_loss"])) <= 1e-2 * kl_rms     # (what a 1e-4 rel-MSE of the terms allows)
    assert abs(float(losses["kl_loss"]) - float(torch.cat(out["kls"], 1).double().mean())) <= 1e-6
    rec, tgt = out["set"].double().cpu(), fwd["pts"].double()
    d = ((rec[:, :, None, :] - tgt[:, None, :, :]) ** 2).sum(-1)                             # [B, n_rec, n_tgt]
    cd = d.min(2)[0].sqrt().mean() + d.min(1)[0].sqrt().mean()                                # CD_loss type 'l1' (evaluation/loss.py:72-79)
    assert abs(float(losses["cd_loss"]) - float(cd)) <= 1e-4 * float(cd)
    # resume: the file layout trainer/base.py `save` writes
    sd = {k: v.clone() for k, v in comp.state_dict().items()}
    changed = {k: (v + 0.25 if v.is_floating_point() else v) for k, v in sd.items()}
    torch.save({"cfg": None, "state_dict": changed, "optim_state_dict": {"state": {}, "param_groups": []}, "scheduler": {},
                "epoch": 40, "itr": 1234, "time": 5.5}, os.path.join(str(tmp_path), "checkpt_40.pth"))
    with open(os.path.join(str(tmp_path), "training.csv"), "w") as f:
        f.write("epoch,itr,loss,time\n20,600,0.5,2\n40,1234,0.4,5\n")
    tr.resume()                                                  # epoch from the last row of training.csv
    assert (tr.epoch, tr.itr, tr.time) == (41, 1234, 5.5)
    assert all(torch.equal(v.detach().cpu(), changed[k].cpu()) for k, v in comp.named_parameters())
    tr.epoch, tr.itr = 1, 0
    tr.resume(epoch=40, finetune=True)                           # weights only
    assert (tr.epoch, tr.itr) == (1, 0)


def test_completion_compressor_trainer_reconstrustion(env, tmp_path):
    ldt = env["ldt"]
    from ldt_amd import ops
    from ldt_amd.metrics import F1Score, L2_ChamferEval_1000
    cfg = copy.deepcopy(env["cfg"])
    cfg.log.save_path = str(tmp_path)
    comp = ldt.Compressor(cfg.compressor)
    comp.load_state_dict(env["csd"], strict=True)
    tr = ldt.CompletionCompressorTrainer(cfg, comp, "cuda:0")
    g = torch.Generator().manual_seed(4)
    loader = [(torch.zeros(2, 3, 8, 8), torch.randn(2, 64, 3, generator=g) * 0.4, torch.randn(2, 32, 3, generator=g)) for _ in range(3)]
    torch.manual_seed(13)
    res = tr.reconstrustion(loader)
    torch.manual_seed(13)
    refs, recs = [], []
    for _, pc, _ in loader:
        pc = pc.cuda().contiguous()
        ref = ops.gather_rows(pc, ops.fps(pc, 64))               # min(2048, 64) points: farthest-point order
        refs.append(ref); recs.append(comp(ref)["set"])
    rec, ref = torch.cat(recs, 0), torch.cat(refs, 0)
    assert set(res) == {"cd", "f1score"}
    assert torch.equal(res["cd"], L2_ChamferEval_1000(rec, ref)) and torch.equal(res["f1score"], F1Score(rec, ref)[0].mean())
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "rec_ep1.npy")), rec.cpu().numpy())


# ------------------------------------------------------------------------------------------------ production width
def test_val_loss_full_width():
    """The Compressor and Score sizes of tests/test_gpu_fullsize.py at B = 64, T = 256: `val_loss` against the torch-CPU fp32/fp64
    restatement fed the GPU's own all_eps and params — the new kernels alone, at the production shape."""
    import ldt_amd
    cfg = ldt_amd.airplane_config(latent_tokens=256, sample_N=100)
    torch.manual_seed(0)
    score = ldt_amd.Score(cfg.score)
    comp = ldt_amd.Compressor(cfg.compressor)
    comp.init()
    tr = ldt_amd.Trainer(cfg, score, comp, "cuda:0")
    B = 64
    g = torch.Generator().manual_seed(8)
    pts = torch.randn(B, 2048, 3, generator=g) * 0.3
    idx = torch.randint(0, cfg.sde.train_N, (B,), generator=g)
    for loss_type in ("l2", "l1"):
        cfg.opt.loss_type = loss_type
        torch.manual_seed(1)
        loss = tr.val_loss({"te_points": pts}, t_index=idx, seed=4242)
        last = {k: v.cpu() for k, v in tr.last_val_loss.items()}
        assert last["eps"].shape == (B, 256, cfg.score.z_dim)
        t = torch.linspace(1.0, cfg.sde.sample_time_eps, cfg.sde.train_N)[idx]
        assert torch.equal(last["t"], t)
        assert torch.equal(last["eta"], ldt_amd.ops.philox_normal(tuple(last["eps"].shape), "cuda", 4242, step=0).cpu())
        xt = last["eps"] * tr.SDE.e2int_f(t)[:, None, None] + sqrt_rn(tr.SDE.var(t))[:, None, None] * last["eta"]
        assert torch.equal(last["xt"], xt)                       # the torch-CPU fp32 expression, bit for bit
        mean64, per64 = dsm_reference(last["eta"], last["params"], None, loss_type == "l1")
        assert relerr(loss, mean64) <= 1e-6 and relerr(last["sample_loss"], per64) <= 1e-6
