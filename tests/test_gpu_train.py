"""GPU (-m gpu): whole Score training steps on the HIP path against tests/golden/score_train_tiny.npz (tools/gen_score_train_golden.py: the
reference's own `Trainer.update_score` on the CPU, and a bf16 twin's distance from it — the yardsticks).

The fixture keeps digests, not tensors (a committed file holds 1 MiB, one copy of the tiny Score is 2.2 MB): the initial weights are rebuilt
from the seed (`torch.manual_seed(21); Score(cfg.score)`, checked against `init_digest::*`), and the reference's iteration-0 gradients are
recomputed with oracle.ldt_oracle.score_forward + autograd in fp32 — which the capture script asserts equal to the reference's to 1e-10
rel-MSE — and tied to the captured ones through `grad0_digest::*`.

Bars: each parameter's gradient rel-MSE <= 2 x max(twin_grad_relmse::<name>, twin_grad_relmse_all), the concatenated gradient <= 2 x
twin_grad_relmse_all, the 20-step loss trajectory's worst relative deviation <= 2 x twin_loss_dev.  The margin of 2: the HIP path rounds at
other places than autocast does (it keeps an fp32 residual stream, fp32 accumulators and fp32 conditioning linears, but rounds P, dS and
every backward GEMM operand to bf16).  Measured values are printed (-s) and recorded in DESIGN.md section 4.11."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rel_mse

pytestmark = pytest.mark.gpu

_CACHE = {}


def golden():
    if "g" not in _CACHE:
        z = np.load(os.path.join(GOLDEN, "score_train_tiny.npz"))
        _CACHE["g"] = {k: (torch.from_numpy(np.asarray(z[k])) if z[k].dtype.kind in "fiu" else z[k]) for k in z.files}
    return _CACHE["g"]


def digest(t):
    t = torch.as_tensor(t).detach().double().cpu().reshape(-1)
    return torch.stack([t.sum(), (t * t).sum(), (t * torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64))).sum()])


def train_cfg(tiny_cfg, num_categorys=1, **opt):
    cfg = copy.deepcopy(tiny_cfg)
    cfg.opt.lr, cfg.opt.warmup_iters, cfg.opt.ema_decay, cfg.opt.grad_norm_clip_value = 2e-3, 5, 0.98, 1.0
    cfg.opt.discrete, cfg.opt.loss_type = True, "l2"
    cfg.data.num_categorys = cfg.score.num_categorys = num_categorys
    for k, v in opt.items():
        setattr(cfg.opt, k, v)
    return cfg


def make_trainer(cfg, tag=""):
    """A trainer on the fixture's initial weights (seed 21) -> (trainer, CPU copy of the initial state_dict)."""
    import ldt_amd
    g = golden()
    torch.manual_seed(21)
    score = ldt_amd.Score(cfg.score)
    init = {k: v.detach().clone() for k, v in score.state_dict().items()}
    for k, v in init.items():
        want, got = g[tag + "init_digest::" + k], digest(v)         # (float64 sums: the summation order differs between hosts)
        assert float((got - want).abs().max()) <= 1e-9 * (float(want[1]) * v.numel()) ** 0.5 + 1e-300, "initial weights differ from the fixture's: " + k
    comp = ldt_amd.Compressor(cfg.compressor)
    comp.init()
    return ldt_amd.Trainer(cfg, score, comp, "cuda"), init


def draw(i):
    """The time indices and the noise of the fixture's iteration i (eta is the first draw after the seed)."""
    g = golden()
    torch.manual_seed(1000 + i)
    return g["idx"][i], torch.randn(g["eps"].shape)


def oracle_loss(sd, cfg, eps, t, e2int_f, var, eta, weight=None, cates=None, l1=False):
    """Latent_SDE_Trainer.py:127-136 over oracle.score_forward, in the dtype of `eps`."""
    from oracle import ldt_oracle as O
    xt = eps * e2int_f[:, None, None] + torch.sqrt(var)[:, None, None] * eta
    lab = None
    if cates is not None:
        lab = O.linear(sd, "LabelEmbedding.mlp.2", F.silu(O.linear(sd, "LabelEmbedding.mlp.0", sd["LabelEmbedding.label_emb.weight"][cates])))
    params = O.score_forward(sd, cfg.score, xt, t, label_emb=lab)
    d = eta - params
    dist = d.abs() if l1 else d * d
    return (dist * (1 if weight is None else weight[:, None, None])).mean()


def oracle_grads(init, cfg, eps, t, e2int_f, var, eta, names, dtype=torch.float32, **kw):
    sd = {k: v.detach().clone().to(dtype) for k, v in init.items()}
    leaves = [sd[n].requires_grad_(True) for n in names]
    c = lambda v: None if v is None else (v.to(dtype) if v.is_floating_point() else v)
    loss = oracle_loss(sd, cfg, c(eps), c(t), c(e2int_f), c(var), c(eta), **{k: (c(v) if torch.is_tensor(v) else v) for k, v in kw.items()})
    loss.backward()
    return {n: p.grad for n, p in zip(names, leaves)}, float(loss)


def reference_grads0(tiny_cfg, tag):
    """Iteration 0's reference gradients, computed once per fixture (unconditional / labelled) and tied to the captured digests."""
    if ("ref", tag) not in _CACHE:
        import ldt_amd
        g = golden()
        cfg = train_cfg(tiny_cfg, 3 if tag else 1)
        torch.manual_seed(21)
        score = ldt_amd.Score(cfg.score)
        init = {k: v.detach().clone() for k, v in score.state_dict().items()}
        names = [n for n, _ in score.named_parameters()]
        sde = ldt_amd.DiffusionVPSDE(cfg.sde)
        torch.manual_seed(1000)
        eta = torch.randn(g["eps"].shape)
        t = torch.linspace(1.0, cfg.sde.sample_time_eps, cfg.sde.train_N).index_select(0, g[tag + "idx"][0])
        grads, loss = oracle_grads(init, cfg, g["eps"], t, sde.e2int_f(t), sde.var(t), eta, names, cates=g[tag + "cates"] if tag else None)
        for n in names:                                        # the captured reference, by digest: [sum, sum of squares, projection]
            want, got = g[tag + "grad0_digest::" + n], digest(grads[n])
            scale = float(want[1].sqrt()) * grads[n].numel() ** 0.5
            assert abs(float(got[1] - want[1])) <= 1e-5 * float(want[1]) and float((got - want)[[0, 2]].abs().max()) <= 1e-5 * scale, n
        assert abs(loss - float(g[tag + "loss"][0])) <= 1e-6 * loss
        for n in names:                                        # the small tensors are stored verbatim: THOSE are the reference
            if tag + "grad0::" + n in g:
                assert rel_mse(grads[n], g[tag + "grad0::" + n]) <= 1e-10, n
                grads[n] = g[tag + "grad0::" + n]
        _CACHE[("ref", tag)] = (grads, names)
    return _CACHE[("ref", tag)]


# ------------------------------------------------------------------------------------------------ gradients of iteration 0
@pytest.mark.parametrize("tag", ["", "lab_"])
def test_iteration0_gradients_and_loss(tiny_cfg, tag):
    g = golden()
    ref, names = reference_grads0(tiny_cfg, tag)
    cfg = train_cfg(tiny_cfg, 3 if tag else 1, grad_norm_clip_value=None)        # no clipping: p.grad stays the raw gradient after the step
    tr, _ = make_trainer(cfg, tag)
    torch.manual_seed(1000)
    eta = torch.randn(g["eps"].shape)
    cates = g[tag + "cates"].cuda() if tag else None
    loss = tr.update_score(g["eps"].cuda(), cates=cates, discrete=True, t_index=g[tag + "idx"][0], eta=eta)
    assert loss.shape == () and loss.is_cuda
    want = float(g[tag + "loss"][0])
    print("%strain loss, iteration 0: %.7f vs the reference's %.7f (relative %.2e)" % (tag, float(loss), want, abs(float(loss) - want) / want))
    assert abs(float(loss) - want) <= 1e-3 * want                                # the bar tests/test_gpu_eval.py holds val_loss to
    named = dict(tr.model.named_parameters())
    assert list(named) == names
    allb = float(g[tag + "twin_grad_relmse_all"])
    worst = 0.0
    for n in names:
        got = named[n].grad
        assert got is not None and got.shape == ref[n].shape and bool(torch.isfinite(got).all()), n
        e, bar = rel_mse(got.cpu(), ref[n]), 2 * max(float(g[tag + "twin_grad_relmse::" + n]), allb)
        worst = max(worst, e / bar)
        assert e <= bar, "%s: gradient rel-MSE %.3e > %.3e (2 x the bf16 twin's)" % (n, e, bar)
    e_all = rel_mse(torch.cat([named[n].grad.reshape(-1) for n in names]).cpu(), torch.cat([ref[n].reshape(-1) for n in names]))
    print("%sgradient rel-MSE, all parameters: %.3e = %.2f x the twin's %.3e; worst per-tensor ratio to its bar %.2f" % (tag, e_all, e_all / allb, allb, worst))
    assert e_all <= 2 * allb


# ------------------------------------------------------------------------------------------------ trajectory, state layout
def run_steps(tr, n, start=0):
    g = golden()
    losses = []
    for i in range(start, start + n):
        idx, eta = draw(i)
        tr.itr = i                                                               # the fixture drives update_score directly: warm-up by itr
        losses.append(tr.update_score(g["eps"].cuda(), discrete=True, t_index=idx, eta=eta))
    return losses


def test_loss_trajectory_and_optimizer_state(tiny_cfg):
    g = golden()
    tr, init = make_trainer(train_cfg(tiny_cfg))
    first = run_steps(tr, 1)
    params = list(tr.model.parameters())
    shapes = [str(s) for s in g["opt_shapes"]]
    assert len(tr.optimizer.state) == len(params) == len(shapes)
    for p, want in zip(params, shapes):                                           # after iteration 1: every entry exists, reference shapes
        st = tr.optimizer.state[p]
        assert sorted(st) == [str(k) for k in g["opt_keys"]]
        assert ";".join("x".join(map(str, v.shape)) for v in (p, st["exp_avg"], st["exp_avg_sq"], st["ema"])) == want
        assert float(st["step"]) == float(g["opt1_step"]) == 1.0
    sd = tr.optimizer.state_dict()
    ref_sd = torch.optim.Adam(params, lr=1e-3).state_dict()
    assert set(sd) == set(ref_sd) and set(sd["param_groups"][0]) - {"initial_lr"} == set(ref_sd["param_groups"][0])
    assert sd["param_groups"][0]["params"] == list(range(len(params))) and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "ema"}
    assert abs(sd["param_groups"][0]["lr"] - 2e-3 / 5) < 1e-12                    # warm-up, iteration 0
    # exp_avg after iteration 1 = 0.1 c g, c the clip factor, against the reference's (stored for the small tensors).  With e_n, e_all the
    # gradient rel-MSEs (held above to bar_n, bar_all) and |c' - c| / c <= | ||g'|| - ||g|| | / ||g|| <= sqrt(e_all), the relative error of
    # c g is at most sqrt(e_n) + sqrt(e_all): rel-MSE <= (sqrt(bar_n) + sqrt(bar_all))^2.
    named = dict(tr.model.named_parameters())
    small = [n for n in named if "exp_avg1::" + n in g]
    assert len(small) == 18                                                       # every bias of the unconditional tiny Score
    allb = float(g["twin_grad_relmse_all"])
    for n in small:
        bar = ((2 * max(float(g["twin_grad_relmse::" + n]), allb)) ** 0.5 + (2 * allb) ** 0.5) ** 2
        e = rel_mse(tr.optimizer.state[named[n]]["exp_avg"].cpu(), g["exp_avg1::" + n])
        assert e <= bar, "%s: exp_avg after iteration 1, rel-MSE %.3e > %.3e" % (n, e, bar)
        # the first Adam step moves every element by lr x sign(g) (m / sqrt(v) = +-1): the EMA equals the new weight, both within lr of the start
        assert torch.equal(tr.optimizer.state[named[n]]["ema"], named[n].data)
        assert float((named[n].data.cpu() - g["after1::" + n]).abs().max()) <= 2 * 2e-3 / 5 * (1 + 1e-5)
    losses = [float(l) for l in first + run_steps(tr, 19, start=1)]
    ref = g["loss"].tolist()
    dev = max(abs(a - b) / b for a, b in zip(losses, ref))
    bar = 2 * float(g["twin_loss_dev"])
    print("20-step loss trajectory: %.4f -> %.4f (reference %.4f -> %.4f); worst relative deviation %.3e = %.2f x the twin's %.3e"
          % (losses[0], losses[-1], ref[0], ref[-1], dev, dev / float(g["twin_loss_dev"]), float(g["twin_loss_dev"])))
    assert losses[-1] < 0.7 * losses[0]                                           # it trains
    assert dev <= bar
    assert abs(tr.optimizer.param_groups[0]["lr"] - 2e-3) < 1e-12 and float(tr.optimizer.state[params[0]]["step"]) == 20.0
    # the optimizer end to end: the 20-step UPDATE (value - initial value) of the small tensors' weights and EMA against the reference's,
    # concatenated, at 2 x the bf16 twin's rel-MSE on the same quantity (Adam's early steps move by ~lr x sign(g): elements whose gradient
    # sign is in doubt differ by whole steps in the twin as well — the yardstick carries that)
    upd = lambda vals, key: (torch.cat([(v.cpu() - init[n]).reshape(-1) for n, v in zip(small, vals)]),
                             torch.cat([(g[key + n] - init[n]).reshape(-1) for n in small]))
    e_w = rel_mse(*upd([named[n].data for n in small], "after20::"))
    e_e = rel_mse(*upd([tr.optimizer.state[named[n]]["ema"] for n in small], "ema20::"))
    print("20-step update of the small tensors: weights rel-MSE %.3e = %.2f x the twin's, EMA %.3e = %.2f x the twin's"
          % (e_w, e_w / float(g["twin_after20_update_relmse"]), e_e, e_e / float(g["twin_ema20_update_relmse"])))
    assert e_w <= 2 * float(g["twin_after20_update_relmse"]) and e_e <= 2 * float(g["twin_ema20_update_relmse"])


def test_step_is_deterministic(tiny_cfg):
    outs = []
    for _ in range(2):
        tr, _ = make_trainer(train_cfg(tiny_cfg))
        run_steps(tr, 2)
        outs.append(([p.grad.clone() for p in tr.model.parameters()], [p.data.clone() for p in tr.model.parameters()],
                     [tr.optimizer.state[p]["ema"].clone() for p in tr.model.parameters()]))
    for a, b in zip(outs[0], outs[1]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_optimizer_readopts_tensors_replaced_from_outside(tiny_cfg):
    """After an EMA swap the parameters live in the second role buffer and the raw weights (as state['ema']) in the first.  Re-pointing
    p.data from outside in that state must not lose either: the optimizer copies both back into its flat buffers, bit for bit."""
    tr, _ = make_trainer(train_cfg(tiny_cfg))
    run_steps(tr, 2)
    opt, params = tr.optimizer, list(tr.model.parameters())
    opt.swap_parameters_with_ema(store_params_in_ema=True)
    want = [(p.data.clone(), opt.state[p]["ema"].clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
    assert all(not torch.equal(w[0], w[1]) for w in want if w[0].numel() > 8)
    for p in params:
        p.data = p.data.clone()                                                  # re-pointed from outside
    F, role, have_ema = opt._ensure_flat()
    assert role == ("a", "b") and have_ema
    for p, o, w in zip(params, F["off"], want):
        st = opt.state[p]
        assert p.data_ptr() == F["a"].data_ptr() + 4 * o and st["ema"].data_ptr() == F["b"].data_ptr() + 4 * o
        assert torch.equal(p.data, w[0]) and torch.equal(st["ema"], w[1]) and torch.equal(st["exp_avg"], w[2]) and torch.equal(st["exp_avg_sq"], w[3])
    opt.state[params[0]]["ema"] = opt.state[params[0]]["ema"].clone()            # one state entry replaced (what a loaded state dict does)
    opt._ensure_flat()
    assert torch.equal(opt.state[params[0]]["ema"], want[0][1]) and opt.state[params[0]]["ema"].data_ptr() == F["b"].data_ptr()
    loss = run_steps(tr, 1, start=2)[0]
    assert bool(torch.isfinite(loss)) and float(opt.state[params[0]]["step"]) == 3.0


# ------------------------------------------------------------------------------------------------ protocol
def _points(cfg, B=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(B, cfg.data.tr_max_sample_points, 3, generator=g)
    pts = pts - pts.mean(1, keepdim=True)
    return pts / pts.norm(dim=-1).amax(1)[:, None, None]


def test_update_protocol_and_sample_sees_the_ema_weights(tiny_cfg):
    """`update` increments itr and leaves the raw (non-EMA) weights in the model; `sample()` after training equals `sample()` of a fresh
    Score loaded with the EMA weights, bit for bit: the packed panels were rebuilt from the swapped-in weights."""
    import ldt_amd
    from oracle import ldt_oracle as O
    cfg = train_cfg(tiny_cfg)
    tr, init = make_trainer(cfg)
    data = {"tr_points": _points(cfg)}
    np.random.seed(5); torch.manual_seed(5)
    for i in range(3):
        loss = tr.update(data)
        assert tr.itr == i + 1 and loss.shape == () and bool(torch.isfinite(loss))
    params = list(tr.model.parameters())
    ema = [tr.optimizer.state[p]["ema"] for p in params]
    assert all(not torch.equal(p.data, e) for p, e in zip(params, ema) if p.numel() > 8)
    assert all(not torch.equal(p.data.cpu(), init[n]) for n, p in tr.model.named_parameters() if p.numel() > 8)
    raw = [p.data.clone() for p in params]
    B, N = 2, cfg.sde.sample_N
    x0, noises = O.draw_noises(99, B, cfg.score.z_scale, cfg.score.z_dim, N)
    pts, eps = tr.sample(B, x0=x0, noise=torch.stack(noises))
    assert all(torch.equal(p.data, r) for p, r in zip(params, raw))               # the swap was undone: raw weights again
    fresh = ldt_amd.Score(cfg.score)
    fresh.load_state_dict({n: e.detach().cpu().clone() for (n, _), e in zip(tr.model.named_parameters(), ema)}, strict=True)
    tr2 = ldt_amd.Trainer(cfg, fresh, tr.compressor, "cuda")
    pts2, eps2 = tr2.sample(B, x0=x0, noise=torch.stack(noises))
    assert torch.equal(eps, eps2) and torch.equal(pts, pts2)


def test_save_resume_reproduces_the_uninterrupted_run(tiny_cfg, tmp_path):
    import ldt_amd
    g = golden()
    cfg = train_cfg(tiny_cfg)
    cfg.log.save_path = str(tmp_path)
    tr, _ = make_trainer(cfg)
    run_steps(tr, 3)
    tr.itr = 3
    path = tr.save()
    ck = torch.load(path, map_location="cpu", weights_only=False)
    ref_ck = torch.load(os.path.join(GOLDEN, "checkpoint_tiny.pth"), map_location="cpu", weights_only=False)
    assert set(ck) == set(ref_ck)
    assert set(ck["score_optim_state_dict"]["state"][0]) == set(ref_ck["score_optim_state_dict"]["state"][0])
    assert set(ck["score_optim_state_dict"]["param_groups"][0]) == set(ref_ck["score_optim_state_dict"]["param_groups"][0])
    idx, eta = draw(3)
    want = tr.update_score(g["eps"].cuda(), discrete=True, t_index=idx, eta=eta)
    tr2 = ldt_amd.Trainer(cfg, ldt_amd.Score(cfg.score), ldt_amd.Compressor(cfg.compressor), "cuda")
    tr2.resume(pretrain=path, load_optim=True)
    assert tr2.itr == 3 and tr2.epoch == tr.epoch + 1
    got = tr2.update_score(g["eps"].cuda(), discrete=True, t_index=idx, eta=eta)
    assert torch.equal(got, want)
    for (n, p), q in zip(tr.model.named_parameters(), tr2.model.parameters()):
        assert torch.equal(p.data, q.data), n
        a, b = tr.optimizer.state[p], tr2.optimizer.state[q]
        assert float(a["step"]) == float(b["step"]) == 4.0
        assert all(torch.equal(a[k], b[k]) for k in ("exp_avg", "exp_avg_sq", "ema")), n


# ------------------------------------------------------------------------------------------------ l1 loss, continuous times
@pytest.mark.parametrize("loss_type,discrete", [("l1", True), ("l2", False)])
def test_l1_loss_and_importance_weighted_times(tiny_cfg, loss_type, discrete):
    """One step each against the oracle's float64 autograd, with the yardstick rule computed here: a bf16 twin (autocast) of the same
    step gives the per-tensor and overall rel-MSE the HIP gradients may be 2 x away from.  discrete=False: iw_quantities draws rho from
    the CPU generator (seeded here) and returns a per-sample weight_p."""
    import ldt_amd
    g = golden()
    cfg = train_cfg(tiny_cfg, loss_type=loss_type, grad_norm_clip_value=None)
    cfg.sde.iw_sample_p_mode = "ll_uniform"                                       # a mode whose weight_p differs per sample
    tr, init = make_trainer(cfg)
    names = [n for n, _ in tr.model.named_parameters()]
    sde = ldt_amd.DiffusionVPSDE(cfg.sde)
    B = g["eps"].shape[0]
    if discrete:
        t = torch.linspace(1.0, cfg.sde.sample_time_eps, cfg.sde.train_N).index_select(0, g["idx"][0])
        e2, var, w, kw = sde.e2int_f(t), sde.var(t), None, dict(t_index=g["idx"][0])
    else:
        torch.manual_seed(4321)
        t, var, e2, w, _, _ = sde.iw_quantities(B, time_eps=cfg.sde.time_eps, iw_sample_mode=cfg.sde.iw_sample_p_mode, iw_subvp_like_vp_sde=False)
        var, e2, w, kw = var.reshape(-1), e2.reshape(-1), w.reshape(-1), {}
        assert float(w.max() - w.min()) > 0
    torch.manual_seed(1000)
    eta = torch.randn(g["eps"].shape)
    ref, ref_loss = oracle_grads(init, cfg, g["eps"], t, e2, var, eta, names, dtype=torch.float64, weight=w, l1=loss_type == "l1")
    sd = {k: v.detach().clone() for k, v in init.items()}
    leaves = [sd[n].requires_grad_(True) for n in names]
    with torch.autocast("cpu", torch.bfloat16):
        oracle_loss(sd, cfg, g["eps"], t.float(), e2.float(), var.float(), eta, weight=None if w is None else w.float(), l1=loss_type == "l1").float().backward()
    twin = {n: rel_mse(p.grad, ref[n]) for n, p in zip(names, leaves)}
    twin_all = rel_mse(torch.cat([p.grad.reshape(-1) for p in leaves]), torch.cat([ref[n].reshape(-1) for n in names]))
    torch.manual_seed(4321)                                                      # the same rho inside update_score
    loss = tr.update_score(g["eps"].cuda(), discrete=discrete, eta=eta, **kw)
    assert abs(float(loss) - ref_loss) <= 1e-3 * ref_loss
    if not discrete:
        assert torch.equal(tr.last_update["weight_p"].cpu(), w.float())
    named = dict(tr.model.named_parameters())
    for n in names:
        e = rel_mse(named[n].grad.cpu(), ref[n])
        assert e <= 2 * max(twin[n], twin_all), "%s: %.3e > 2 x max(%.3e, %.3e)" % (n, e, twin[n], twin_all)
    e_all = rel_mse(torch.cat([named[n].grad.reshape(-1) for n in names]).cpu(), torch.cat([ref[n].reshape(-1) for n in names]))
    print("%s discrete=%s: gradient rel-MSE %.3e = %.2f x the twin's %.3e" % (loss_type, discrete, e_all, e_all / twin_all, twin_all))
    assert e_all <= 2 * twin_all
