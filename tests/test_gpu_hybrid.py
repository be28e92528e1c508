"""GPU (-m gpu): the hybrid trainer's evaluation on the HIP path — ldt_nelbo_terms, `HybridTrainer.val_nelbo` against
tests/golden/hybrid_nelbo_tiny.npz (the reference's KL term of `clc_compressor`, draws injected; captured by
tools/golden/gen_hybrid_eval_golden.py), `sample` / `valsample` / `valrecon` / `resume` against `ldt_amd.Trainer` and upstream's
file names and counts."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_mse

pytestmark = pytest.mark.gpu

CASES = [("vpsde", "discrete"), ("vpsde", "ll_uniform"), ("vpsde", "ll_iw"), ("sub_vpsde", "ll_iw"), ("vesde", "ll_iw")]


def nelbo_golden():
    z = np.load(os.path.join(GOLDEN, "hybrid_nelbo_tiny.npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("shape", [(64, 256, 120), (5, 7, 11), (3, 4, 6)])
@pytest.mark.parametrize("weighted", [False, True])
def test_nelbo_terms_kernel(shape, weighted):
    """(64, 256, 120): B x per_sample of the headline shape, 16-byte accesses; (5, 7, 11): per_sample = 77, the scalar form; (3, 4, 6): fewer
    elements than threads.  Against the float64 evaluation on the kernel's own inputs, at the bar test_gpu_eval.py holds ldt_dsm_loss to."""
    from ldt_amd import ops
    g = torch.Generator().manual_seed(17)
    eta, params = torch.randn(shape, generator=g), torch.randn(shape, generator=g) * 0.7
    logqz = -0.9189385332 - 0.5 * (torch.randn(shape, generator=g) * 1.5 - 1.0) - 0.5 * torch.randn(shape, generator=g) ** 2
    w = (torch.rand(shape[0], generator=g) * 30.0 + 0.05) if weighted else None
    B = shape[0]
    tot, per = ops.nelbo_terms(eta.cuda(), params.cuda(), logqz.cuda(), None if w is None else w.cuda())
    assert tot.shape == (2,) and per.shape == (B, 2) and tot.is_cuda and tot.dtype == torch.float32
    dist = (eta.double() - params.double()) ** 2
    if w is not None:
        dist = dist * w.double().view(-1, 1, 1)
    want_per = torch.stack([dist.reshape(B, -1).sum(1), logqz.double().reshape(B, -1).sum(1)], 1)
    print("nelbo_terms %s weighted=%s: relerr per sample %.2e, batch %.2e" % (shape, weighted, relerr(per, want_per), relerr(tot, want_per.sum(0))))
    assert relerr(per, want_per) <= 1e-6 and relerr(tot, want_per.sum(0)) <= 1e-6
    tot2, per2 = ops.nelbo_terms(eta.cuda(), params.cuda(), logqz.cuda(), None if w is None else w.cuda())
    assert torch.equal(tot2, tot) and torch.equal(per2, per)                                 # fixed summation order
    with pytest.raises(ValueError):
        ops.nelbo_terms(eta.cuda(), params.cuda(), logqz.cuda()[:, :1])
    with pytest.raises(ValueError):
        ops.nelbo_terms(eta.cuda(), params.cuda(), logqz.cuda(), torch.ones(B + 1, device="cuda"))


# ------------------------------------------------------------------------------------------------ tiny fixture
def _cfg(tiny_cfg, g, sde_type, mode):
    c = copy.deepcopy(tiny_cfg)
    c.sde.sde_type = sde_type
    for k in ("sigma2_min", "sigma2_max", "sigma2_0"):
        if "%s/%s" % (sde_type, k) in g:
            setattr(c.sde, k, float(g["%s/%s" % (sde_type, k)]))
    c.opt.discrete = mode == "discrete"
    if mode != "discrete":
        c.sde.iw_sample_q_mode = mode
    return c


def _trainer(cfg, cls=None):
    import ldt_amd
    _, ssd = load_golden("score_tiny")
    _, csd = load_golden("trainer_sample_tiny")
    score = ldt_amd.Score(cfg.score)
    score.load_state_dict(ssd["w"], strict=True)
    comp = ldt_amd.Compressor(cfg.compressor)
    comp.load_state_dict(csd["c"], strict=True)
    return (cls or ldt_amd.HybridTrainer)(cfg, score, comp, "cuda:0")


@pytest.mark.parametrize("sde_type,mode", CASES)
def test_val_nelbo_golden(tiny_cfg, sde_type, mode):
    """Injected rho / t_index / eta / posterior noise: the reference's KL term, and its pieces element by element."""
    g = nelbo_golden()
    tag = "%s/%s" % (sde_type, mode)
    cfg = _cfg(tiny_cfg, g, sde_type, mode)
    tr = _trainer(cfg)
    data = {"te_points": g["pts"], "cate_idx": torch.zeros(g["pts"].shape[0], dtype=torch.long)}
    res = tr.val_nelbo(data, rho=g[tag + "/rho"], t_index=g["idx"], eta=g["eta"], post_noise=list(g["post_noise"]))
    assert set(res) == {"kl", "logqz", "score_term", "cross_entropy_const", "rec_cd"}
    assert all(v.shape == () and v.is_cuda for v in res.values())
    last = tr.last_val_nelbo
    B = g["pts"].shape[0]
    # the times and weights are the host iw_quantities result (or the discrete grid's), bit for bit
    if mode == "discrete":
        t = torch.linspace(1.0, cfg.sde.sample_time_eps, cfg.sde.train_N).index_select(0, g["idx"].long())
        w = tr.SDE.g2(t) / (2 * tr.SDE.var(t))
    else:
        t, _, _, w, _, _ = tr.SDE.iw_quantities(B, cfg.sde.time_eps, mode, sde_type == "sub_vpsde", rho=g[tag + "/rho"])
    assert torch.equal(last["t"].cpu(), t) and torch.equal(last["weight_q"].cpu(), w.reshape(-1))
    assert float((t - g[tag + "/t"]).abs().max()) <= 1e-6 and relerr(w.reshape(-1), g[tag + "/weight_q"]) <= 1e-4
    e = {k: rel_mse(last[k].cpu(), g[k if k == "logqz" else tag + "/" + k]) for k in ("xt", "params", "logqz")}
    # |kl - golden| <= 1e-2 x rms of the golden's per-element (logqz - logpz) terms: what a 1e-4 rel-MSE of the terms allows
    c = float(g[tag + "/cross_entropy_const"])
    terms = g["logqz"].double() + (g["eta"].double() - g[tag + "/params"].double()) ** 2 * g[tag + "/weight_q"].double().view(-1, 1, 1) + c
    rms = float(terms.pow(2).mean().sqrt())
    assert abs(float(terms.mean()) - float(g[tag + "/kl_loss"])) <= 1e-5 * rms                # (the fixture is consistent with itself)
    print("val_nelbo %s: rel-MSE xt %.3e params %.3e logqz %.3e; kl %.6f vs the reference's %.6f (|diff| %.3e, bar %.3e)" % (
        tag, e["xt"], e["params"], e["logqz"], float(res["kl"]), float(g[tag + "/kl_loss"]), abs(float(res["kl"]) - float(g[tag + "/kl_loss"])),
        1e-2 * rms))
    assert e["xt"] <= 1e-4 and e["params"] <= 1e-4 and e["logqz"] <= 1e-4
    assert abs(float(res["kl"]) - float(g[tag + "/kl_loss"])) <= 1e-2 * rms
    assert abs(float(res["cross_entropy_const"]) - c) <= 1e-6 * max(abs(c), 1.0)
    # the returned pieces add up, and are the float64 sums of the kernel's own inputs
    assert abs(float(res["kl"]) - (float(res["logqz"]) + float(res["score_term"]) + float(res["cross_entropy_const"]))) <= 1e-5 * max(1.0, abs(float(res["kl"])))
    own = (last["eta"].double() - last["params"].double()) ** 2 * last["weight_q"].double().view(-1, 1, 1)
    assert relerr(res["score_term"], own.mean()) <= 1e-6 and relerr(res["logqz"], last["logqz"].double().mean()) <= 1e-6
    assert rel_mse(last["set"].cpu(), g["set"]) <= 1e-4 and bool(torch.isfinite(res["rec_cd"])) and float(res["rec_cd"]) > 0


def test_val_nelbo_ema_swap_seeding_and_default_draws(tiny_cfg):
    g = nelbo_golden()
    cfg = _cfg(tiny_cfg, g, "vpsde", "ll_iw")
    tr = _trainer(cfg)
    data = {"te_points": g["pts"]}

    def run(**kw):
        torch.manual_seed(3)                                     # keys the posterior noise, rho, and eta when no seed is given
        return tr.val_nelbo(data, **kw)["kl"]

    base = run(seed=77)
    assert torch.equal(run(seed=77), base)                       # same seeds: the same figure, bit for bit
    assert not torch.equal(run(seed=78), base)
    # default draws: posterior noise, then ONE torch.rand(B) for rho — the times iw_quantities gives for it
    torch.manual_seed(3)
    tr.compressor(g["pts"].cuda())
    rho = torch.rand(g["pts"].shape[0])
    assert torch.equal(tr.last_val_nelbo["t"].cpu(), tr.SDE.iw_quantities(2, cfg.sde.time_eps, "ll_iw", False, rho=rho)[0])
    # `discrete=` overrides cfg.opt.discrete: numpy's global generator over the training grid
    np.random.seed(11)
    want_idx = np.random.choice(np.arange(cfg.sde.train_N), 2, replace=True)
    np.random.seed(11)
    run(discrete=True, seed=5)
    assert torch.equal(tr.last_val_nelbo["t"].cpu(), torch.linspace(1.0, cfg.sde.sample_time_eps, cfg.sde.train_N)[torch.from_numpy(want_idx)])
    with pytest.raises(ValueError):
        run(discrete=True, t_index=[1], seed=5)
    # EMA weights are what is evaluated, and the model's own weights are back afterwards — also when the Score call raises
    before = [p.data.clone() for p in tr.model.parameters()]
    for p in tr.model.parameters():
        tr.optimizer.state[p] = {"ema": p.data * 0.5}
    assert not torch.equal(run(seed=77), base)
    restored = lambda: (all(torch.equal(p.data, b) for p, b in zip(tr.model.parameters(), before)) and
                        all(torch.equal(tr.optimizer.state[p]["ema"], b * 0.5) for p, b in zip(tr.model.parameters(), before)))
    assert restored()
    def boom(*a, **k):
        raise RuntimeError("score call failed")

    tr.model.forward = boom
    try:
        with pytest.raises(RuntimeError, match="score call failed"):
            run(seed=77)
    finally:
        del tr.model.forward
    assert restored()
    tr.optimizer.state.clear()
    assert torch.equal(run(seed=77), base)
    # 'drop_all_uniform': one shared (1, 1) weight, broadcast over the batch
    c2 = _cfg(tiny_cfg, g, "vpsde", "drop_all_uniform")
    tr2 = _trainer(c2)
    torch.manual_seed(3)
    r2 = tr2.val_nelbo(data, seed=77)
    assert torch.equal(tr2.last_val_nelbo["weight_q"].cpu(), torch.ones(2)) and bool(torch.isfinite(r2["kl"]))
    # the label path (cfg.data.num_categorys > 1 reads data['cate_idx']) on a label-conditional Score
    import ldt_amd
    c3 = copy.deepcopy(cfg)
    c3.data.num_categorys, c3.score.num_categorys = 3, 3
    torch.manual_seed(0)
    tr3 = ldt_amd.HybridTrainer(c3, ldt_amd.Score(c3.score), tr.compressor, "cuda:0")
    d0 = dict(data, cate_idx=torch.zeros(2, dtype=torch.long))
    d1 = dict(data, cate_idx=torch.ones(2, dtype=torch.long))
    torch.manual_seed(3); k0 = tr3.val_nelbo(d0, seed=5)["kl"]
    torch.manual_seed(3); k1 = tr3.val_nelbo(d1, seed=5)["kl"]
    assert bool(torch.isfinite(k0)) and not torch.equal(k0, k1)


# ------------------------------------------------------------------------------------------------ sampling and the loops
def test_sample_returns_points_only_and_equals_trainer_sample(tiny_cfg, capsys):
    import ldt_amd
    hy = _trainer(copy.deepcopy(tiny_cfg))
    tr = _trainer(copy.deepcopy(tiny_cfg), ldt_amd.Trainer)
    torch.manual_seed(12)
    pts = hy.sample(3, seed=99)
    out = capsys.readouterr().out
    torch.manual_seed(12)
    want, want_eps = tr.sample(3, seed=99)
    assert torch.is_tensor(pts) and pts.shape == (3, tiny_cfg.data.tr_max_sample_points, 3)
    assert torch.equal(pts, want) and torch.equal(hy.last_eps, want_eps)
    line = [ln for ln in out.splitlines() if ln.startswith("NFE:")]
    assert len(line) == 1 and line[0].startswith("NFE:%d, NFEs" % tiny_cfg.sde.sample_N) and line[0].endswith("/s")
    # the score function is Trainer's
    t, x = torch.full((3,), 0.5, device="cuda"), torch.randn(3, tiny_cfg.score.z_scale, tiny_cfg.score.z_dim).cuda()
    s_h, p_h = hy.score_fn(t, x)
    s_t, p_t = tr.score_fn(t, x)
    assert torch.equal(s_h, s_t) and torch.equal(p_h, p_t)
    # the probability-flow ODE mode goes through sample_model_ode and reports its own NFE count
    c = copy.deepcopy(tiny_cfg)
    c.sde.sample_mode, c.sde.ode_tol = "continuous", 1e-2
    hy2, tr2 = _trainer(c), _trainer(copy.deepcopy(c), ldt_amd.Trainer)
    torch.manual_seed(4)
    p2 = hy2.sample(2)
    out = capsys.readouterr().out
    torch.manual_seed(4)
    assert torch.equal(p2, tr2.sample(2)[0])
    assert ("NFE:%d, NFEs" % hy2.nfe_count) in out and hy2.nfe_count > 0


def _loader(n_batches, B, N, cates=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n_batches):
        d = {"te_points": torch.randn(B, N, 3, generator=g) * 0.4, "tr_points": torch.randn(B, N, 3, generator=g) * 0.4,
             "shift": torch.randn(B, 1, 3, generator=g), "scale": torch.rand(B, 1, 1, generator=g) + 0.5,
             "mean": torch.randn(B, 1, 3, generator=g), "std": torch.rand(B, 1, 1, generator=g) + 0.5,
             "cate_idx": torch.zeros(B, dtype=torch.long) if cates is None else cates[i]}
        out.append(d)
    return out


def test_valsample_and_valrecon_single_category(tiny_cfg, tmp_path):
    from ldt_amd.metrics import compute_all_metrics
    cfg = copy.deepcopy(tiny_cfg)
    cfg.log.save_path = str(tmp_path)
    hy = _trainer(cfg)
    loader = _loader(2, 3, 64)
    torch.manual_seed(6)
    res = hy.valsample(loader)
    smp = hy.last_valsample["samples"]
    assert smp.shape == (6, 64, 3)
    assert os.listdir(str(tmp_path)) == ["smp{:}_ep1.npy"]                                   # upstream's literal name (:228 fills only the %d)
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "smp{:}_ep1.npy")), smp.cpu().numpy())
    ref = torch.cat([d["te_points"] for d in loader], 0).cuda()
    want = compute_all_metrics(smp, ref, batch_size=64)
    assert set(res) == {"val/gen/%s" % k for k in want} and all(isinstance(v, float) for v in res.values())
    for k, v in want.items():
        assert res["val/gen/%s" % k] == (v if isinstance(v, float) else v.item()), k
    # valrecon: compressor(ref_pts), de-normalised by shift / scale
    torch.manual_seed(9)
    res = hy.valrecon(loader)
    torch.manual_seed(9)
    rec = torch.cat([hy.compressor(d["te_points"].cuda())["set"] * d["scale"].cuda() + d["shift"].cuda() for d in loader], 0)
    ref = torch.cat([d["te_points"].cuda() * d["scale"].cuda() + d["shift"].cuda() for d in loader], 0)
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "rec_ep1.npy")), rec.cpu().numpy())
    want = compute_all_metrics(rec, ref, batch_size=256)
    assert set(res) == {"val/gen/%s" % k for k in want}
    for k, v in want.items():
        assert res["val/gen/%s" % k] == (v if isinstance(v, float) else v.item()), k


def test_valsample_and_valrecon_multi_category(tiny_cfg, tmp_path):
    """Five shapes of the category at test_batch_size 3: two sampled batches (6 clouds, not cut to 5) and encodes of 3 and 2 shapes."""
    import ldt_amd
    from ldt_amd.metrics import compute_all_metrics
    cfg = copy.deepcopy(tiny_cfg)
    cfg.log.save_path = str(tmp_path)
    cfg.data.num_categorys, cfg.score.num_categorys, cfg.data.test_batch_size = 3, 3, 3
    _, csd = load_golden("trainer_sample_tiny")
    torch.manual_seed(0)
    comp = ldt_amd.Compressor(cfg.compressor)
    comp.load_state_dict(csd["c"], strict=True)
    hy = ldt_amd.HybridTrainer(cfg, ldt_amd.Score(cfg.score), comp, "cuda:0")
    loader = _loader(2, 4, 64, cates=[torch.tensor([2, 0, 2, 2]), torch.tensor([2, 1, 2, 0])])
    torch.manual_seed(6)
    res = hy.valsample(loader, val_cate=2)
    smp, ref = hy.last_valsample["samples"], hy.last_valsample["refs"]
    assert ref.shape[0] == 5 and smp.shape[0] == 6                                          # ceil(5 / 3) batches of 3, NOT cut to len(ref) (:223-224)
    assert np.load(os.path.join(str(tmp_path), "smp{:}_ep1.npy")).shape == (6, 64, 3)
    want = compute_all_metrics(smp, ref, batch_size=64)
    assert set(res) == {"val/gen/%s" % k for k in want} and "val/gen/1-NN-CD-acc" in res
    # valrecon: the shapes of the category, re-batched by test_batch_size, de-normalised by mean / std.  The Compressor calls are
    # recorded as the trainer makes them: what it encodes, and that the dump and the metrics are made of what came back.
    keep = [d["cate_idx"] == 2 for d in loader]
    pts = torch.cat([d["te_points"][k] for d, k in zip(loader, keep)], 0).cuda()
    sh = torch.cat([d["mean"][k] for d, k in zip(loader, keep)], 0).cuda()
    sc = torch.cat([d["std"][k] for d, k in zip(loader, keep)], 0).cuda()
    calls = []
    real_forward = hy.compressor.forward

    def recording_forward(x, *a, **k):
        out = real_forward(x, *a, **k)
        calls.append((x.clone(), a, k, out["set"].clone()))
        return out

    hy.compressor.forward = recording_forward
    try:
        res = hy.valrecon(loader, val_cate=2)
    finally:
        del hy.compressor.forward
    assert [c[0].shape[0] for c in calls] == [3, 2] and all(c[1] == () and c[2] == {} for c in calls)      # no label, as upstream (:289)
    assert torch.equal(torch.cat([c[0] for c in calls], 0), pts)
    rec = torch.cat([c[3] for c in calls], 0) * sc + sh
    assert torch.equal(hy.last_valrecon["rec"], rec) and torch.equal(hy.last_valrecon["ref"], pts * sc + sh)
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "rec_ep1.npy")), rec.cpu().numpy())
    want = compute_all_metrics(rec, pts * sc + sh, batch_size=256)
    assert set(res) == {"val/gen/%s" % k for k in want}
    for k, v in want.items():
        assert res["val/gen/%s" % k] == (v if isinstance(v, float) else v.item()), k
    with pytest.raises(ValueError):
        hy.valsample(loader, val_cate=5)


def test_resume_then_sample_equals_trainer(tmp_path):
    """A checkpoint written by the reference's `save` is resumed like `ldt_amd.Trainer` resumes it (EMA from `score_optim_state_dict`); the
    compressor optimizer / scheduler entries, which this file does not hold, are not asked for."""
    import ldt_amd
    path = os.path.join(GOLDEN, "checkpoint_tiny.pth")
    a, _ = load_golden("checkpoint_tiny_expect")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    cfg = ck["cfg"]
    assert "compressor_optim_state_dict" not in ck
    torch.manual_seed(9)
    hy = ldt_amd.HybridTrainer(cfg, ldt_amd.Score(cfg.score), ldt_amd.Compressor(cfg.compressor), "cuda:0")
    hy.resume(pretrain=path, strict=True)
    torch.manual_seed(9)
    tr = ldt_amd.Trainer(cfg, ldt_amd.Score(cfg.score), ldt_amd.Compressor(cfg.compressor), "cuda:0")
    tr.resume(pretrain=path, strict=True)
    assert (hy.epoch, hy.itr, hy.time) == (tr.epoch, tr.itr, tr.time) == (ck["epoch"] + 1, ck["itr"], ck["time"])
    pts = hy.sample(2, x0=a["x0"], noise=a["noises"])
    want, want_eps = tr.sample(2, x0=a["x0"], noise=a["noises"])
    assert torch.equal(pts, want) and rel_mse(hy.last_eps.cpu(), a["eps"]) < 1e-4          # the EMA weights were adopted
    # load_optim=False: raw weights; finetune: epoch 1, itr 0; the reference's file layout under cfg.log.save_path
    c2 = copy.deepcopy(cfg)
    c2.log.save_path = str(tmp_path)
    full = dict(ck, compressor_optim_state_dict={"state": {}, "param_groups": []}, compressor_scheduler={})
    torch.save(full, os.path.join(str(tmp_path), "checkpt_%d.pth" % ck["epoch"]))
    with open(os.path.join(str(tmp_path), "training.csv"), "w") as f:
        f.write("epoch,itr,loss_score,kl,rec,time\n%d,%d,0.5,0.1,0.2,2\n" % (ck["epoch"], ck["itr"]))
    hy2 = ldt_amd.HybridTrainer(c2, ldt_amd.Score(cfg.score), ldt_amd.Compressor(cfg.compressor), "cuda:0")
    hy2.resume(load_optim=False)                                 # epoch from the last row of training.csv
    assert hy2.epoch == ck["epoch"] + 1 and not hy2.optimizer.state
    hy2.sample(2, x0=a["x0"], noise=a["noises"])
    assert rel_mse(hy2.last_eps.cpu(), a["eps_raw_weights"]) < 1e-4
    hy2.resume(epoch=ck["epoch"], finetune=True)
    assert (hy2.epoch, hy2.itr) == (1, 0)
    # load_pretrain: cfg.opt.pretrain_path, both state dicts, strict
    c2.opt.pretrain_path = os.path.join(str(tmp_path), "checkpt_%d.pth" % ck["epoch"])
    hy3 = ldt_amd.HybridTrainer(c2, ldt_amd.Score(cfg.score), ldt_amd.Compressor(cfg.compressor), "cuda:0")
    hy3.load_pretrain()
    assert all(torch.equal(v.detach().cpu(), ck["score_state_dict"][k]) for k, v in hy3.model.named_parameters())
