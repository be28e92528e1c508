"""GPU (-m gpu): whole Score training steps on a ViPC condition pair through `CompletionTrainer.update_score`, against
tests/golden/score_train_cond.npz (tools/gen_score_train_cond_golden.py: the reference's own completion `Trainer.update_score` with a
condition tuple on the CPU, its gradient with respect to the pair, and a bf16 twin's distance from it — the yardsticks).  Helpers:
tests/train_cond_checks.py.

Bars, those of tests/test_gpu_train.py for their reason: the loss of iteration 0 within 1e-3 relative of the reference's; each parameter's
gradient rel-MSE <= 2 x max(twin_grad_relmse::<name>, twin_grad_relmse_all), the concatenated gradient <= 2 x twin_grad_relmse_all; the
gradient with respect to pts_condition / img_condition <= 2 x max(twin_dcond_relmse::<which>, twin_grad_relmse_all); the 20-step loss
trajectory's worst relative deviation <= 2 x twin_loss_dev.  The margin of 2: the HIP path rounds at other places than autocast does (it
keeps an fp32 residual stream, fp32 accumulators and fp32 conditioning linears, but rounds P, dS at head widths 32 and 64, the condition
tokens and every backward GEMM operand to bf16).  Measured values are printed (-s) and recorded in DESIGN.md section 4.14.

Before the conditioned step existed every test here ended at refuse_untrainable ("ViPC / point condition") or at `CompletionTrainer.update`."""
import copy

import pytest
import torch

import train_cond_checks as tc
import train_tape as tt
from conftest import rel_mse

pytestmark = pytest.mark.gpu


def make_trainer(cfg, key):
    import ldt_amd
    score, init = tc.initial_score(cfg, key)
    comp = ldt_amd.Compressor(cfg.compressor)
    comp.init()
    return ldt_amd.CompletionTrainer(cfg, score, comp, "cuda"), init


def pair_on_device(key):
    eps, pts, img = tc.inputs_of(key)
    return eps.cuda(), (pts.cuda(), img.cuda())


# ------------------------------------------------------------------------------------------------ iteration 0 against the reference
@pytest.mark.parametrize("key", list(tc.MODELS))
def test_iteration0_gradients_loss_and_condition_gradients(tiny_cfg, key):
    g = tc.golden()
    ref, names, ref_pts, ref_img, _ = tc.reference_grads0(tiny_cfg, key)
    tr, _ = make_trainer(tc.train_cfg(tiny_cfg, key, grad_norm_clip_value=None), key)     # no clipping: p.grad stays the raw gradient
    eps, pair = pair_on_device(key)
    idx, eta = tc.draw(key, 0)
    cates = None if tc.cates_of(key) is None else tc.cates_of(key).cuda()
    loss = tr.update_score(eps, condition=pair, cates=cates, discrete=True, t_index=idx, eta=eta)
    assert loss.shape == () and loss.is_cuda
    want = float(g[key + "_loss"][0])
    print("%s: train loss, iteration 0: %.7f vs the reference's %.7f (relative %.2e)" % (key, float(loss), want, abs(float(loss) - want) / want))
    assert abs(float(loss) - want) <= 1e-3 * want
    named = dict(tr.model.named_parameters())
    assert list(named) == names
    allb = float(g[key + "_twin_grad_relmse_all"])
    worst = 0.0
    for n in names:
        got = named[n].grad
        assert got is not None and got.shape == ref[n].shape and bool(torch.isfinite(got).all()), n
        e, bar = rel_mse(got.cpu(), ref[n]), 2 * max(float(g[key + "_twin_grad_relmse::" + n]), allb)
        worst = max(worst, e / bar)
        assert e <= bar, "%s: gradient rel-MSE %.3e > %.3e (2 x the bf16 twin's)" % (n, e, bar)
    e_all = rel_mse(torch.cat([named[n].grad.reshape(-1) for n in names]).cpu(), torch.cat([ref[n].reshape(-1) for n in names]))
    print("%s: gradient rel-MSE, all parameters: %.3e = %.2f x the twin's %.3e; worst per-tensor ratio to its bar %.2f" % (key, e_all, e_all / allb, allb, worst))
    assert e_all <= 2 * allb
    # the gradient handed back for ConditionNet's backward
    d_pts, d_img = tr.last_condition_grad
    assert d_pts.dtype == torch.float32 and d_pts.is_cuda and tuple(d_pts.shape) == tuple(ref_pts.shape) and d_pts.is_contiguous()
    tw = float(g[key + "_twin_dcond_relmse::pts"])
    e = rel_mse(d_pts.cpu(), ref_pts)
    print("%s: d loss / d pts_condition rel-MSE %.3e = %.2f x the twin's %.3e" % (key, e, e / tw, tw))
    assert e <= 2 * max(tw, allb)
    if key == "z":                                            # a label and a condition: the image condition was dropped (score.py:135)
        assert d_img is None and ref_img is None
    else:
        assert d_img.dtype == torch.float32 and tuple(d_img.shape) == tuple(ref_img.shape)
        tw = float(g[key + "_twin_dcond_relmse::img"])
        e = rel_mse(d_img.cpu(), ref_img)
        print("%s: d loss / d img_condition rel-MSE %.3e = %.2f x the twin's %.3e" % (key, e, e / tw, tw))
        assert e <= 2 * max(tw, allb)


def test_loss_trajectory_of_twenty_steps(tiny_cfg):
    g = tc.golden()
    tr, _ = make_trainer(tc.train_cfg(tiny_cfg, "x"), "x")
    eps, pair = pair_on_device("x")
    losses = []
    for i in range(tc.MODELS["x"]["iters"]):
        idx, eta = tc.draw("x", i)
        tr.itr = i                                            # the fixture drives update_score directly: warm-up by itr
        losses.append(tr.update_score(eps, condition=pair, discrete=True, t_index=idx, eta=eta))
    losses = [float(l) for l in losses]
    ref = g["x_loss"].tolist()
    dev, tw = max(abs(a - b) / b for a, b in zip(losses, ref)), float(g["x_twin_loss_dev"])
    print("x: 20-step loss trajectory: %.4f -> %.4f (reference %.4f -> %.4f); worst relative deviation %.3e = %.2f x the twin's %.3e"
          % (losses[0], losses[-1], ref[0], ref[-1], dev, dev / tw, tw))
    assert losses[-1] < 0.7 * losses[0]                       # it trains
    assert dev <= 2 * tw
    assert abs(tr.optimizer.param_groups[0]["lr"] - 2e-3) < 1e-12 and float(tr.optimizer.state[next(iter(tr.model.parameters()))]["step"]) == 20.0


# ------------------------------------------------------------------------------------------------ ScoreTrainStep driven directly, ragged sizes
RAGGED = dict(hidden=256, heads=4, blocks=3, B=3, T=72, S=40)
_RAGGED = {}


def ragged_case(tiny_cfg):
    """Hidden 256 / 4 heads / 3 blocks, B 3 x T 72 (216 rows: no multiple of 64), S 40 (120 condition rows) -> the model on the CPU, its
    inputs, and once: float64 oracle autograd (the reference) and the bf16 twin's distances from it (the yardsticks)."""
    if not _RAGGED:
        from oracle import ldt_oracle as O
        r = RAGGED
        model, x, t, _, eta = tt.make_case(tiny_cfg.score, r["hidden"], r["heads"], r["blocks"], r["B"], r["T"], 1, None)
        g = torch.Generator().manual_seed(91)
        pts, img = torch.randn(r["B"], r["hidden"], r["S"], generator=g) * 0.5, torch.randn(r["B"], model.t_dim, generator=g) * 0.5
        init = {k: v.detach().clone() for k, v in model.state_dict().items()}
        names = [n for n, _ in model.named_parameters()]

        def run(dtype, autocast):
            c = lambda v: v.detach().clone().to(dtype)
            sd = {k: c(v) for k, v in init.items()}
            leaves = [sd[n].requires_grad_(True) for n in names]
            p, im = c(pts).requires_grad_(True), c(img).requires_grad_(True)
            with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
                out = O.score_forward(sd, model.cfg, c(x), c(t), condition=(p.transpose(1, 2), im)).float()
            d = c(eta).to(out.dtype) - out
            (d * d).mean().backward()
            return out.detach(), {n: q.grad for n, q in zip(names, leaves)}, p.grad, im.grad

        out64, ref, rp, ri = run(torch.float64, False)
        out_t, tw, tp, ti = run(torch.float32, True)
        cat = lambda d: torch.cat([d[n].reshape(-1) for n in names])
        _RAGGED.update(model=model, x=x, t=t, eta=eta, pts=pts, img=img, names=names, out=out64, ref=ref, ref_pts=rp, ref_img=ri,
                       twin={n: rel_mse(tw[n], ref[n]) for n in names}, twin_all=rel_mse(cat(tw), cat(ref)), twin_out=rel_mse(out_t, out64),
                       twin_pts=rel_mse(tp, rp), twin_img=rel_mse(ti, ri))
    return _RAGGED


def ragged_step(c, dparams_mask=None):
    """One forward + backward of a fresh device copy of the model -> (params, {name: grad}, (d_pts, d_img))."""
    import ldt_amd.train as train
    model = copy.deepcopy(c["model"]).cuda()
    tt.flat_grads(model)
    step = train.ScoreTrainStep(model, allow_condition=True)
    params = step.forward(c["x"].cuda(), c["t"].cuda(), condition=(c["pts"].cuda(), c["img"].cuda()))
    assert step.saved is not None and sorted(k for k in step.saved["blocks"][0] if k in ("q", "kv", "qkv", "o")) == ["kv", "o", "q"]
    assert sorted(k for k in step.saved["blocks"][1] if k in ("q", "kv", "qkv", "o")) == ["o", "qkv"]
    dparams = train.ops.dsm_loss_bwd(c["eta"].cuda(), params)
    if dparams_mask is not None:
        dparams = dparams * dparams_mask
    dcond = step.backward(dparams)
    assert step.saved is None and dcond is step.dcondition
    return params, {n: p.grad.clone() for n, p in model.named_parameters()}, dcond


def test_ragged_sizes_against_float64_autograd(tiny_cfg):
    c = ragged_case(tiny_cfg)
    params, grads, (d_pts, d_img) = ragged_step(c)
    e = rel_mse(params.cpu(), c["out"])
    print("ragged: output rel-MSE %.3e = %.2f x the twin's %.3e" % (e, e / c["twin_out"], c["twin_out"]))
    assert e <= 2 * c["twin_out"]
    worst = 0.0
    for n in c["names"]:
        e, bar = rel_mse(grads[n].cpu(), c["ref"][n]), 2 * max(c["twin"][n], c["twin_all"])
        worst = max(worst, e / bar)
        assert e <= bar, "%s: gradient rel-MSE %.3e > %.3e" % (n, e, bar)
    e_all = rel_mse(torch.cat([grads[n].reshape(-1) for n in c["names"]]).cpu(), torch.cat([c["ref"][n].reshape(-1) for n in c["names"]]))
    print("ragged: gradient rel-MSE, all parameters: %.3e = %.2f x the twin's %.3e; worst per-tensor ratio to its bar %.2f"
          % (e_all, e_all / c["twin_all"], c["twin_all"], worst))
    assert e_all <= 2 * c["twin_all"]
    r = RAGGED
    assert tuple(d_pts.shape) == (r["B"], r["hidden"], r["S"]) and tuple(d_img.shape) == tuple(c["img"].shape)
    for nm, got, ref, tw in (("pts", d_pts, c["ref_pts"], c["twin_pts"]), ("img", d_img, c["ref_img"], c["twin_img"])):
        e = rel_mse(got.cpu(), ref)
        print("ragged: d loss / d %s_condition rel-MSE %.3e = %.2f x the twin's %.3e" % (nm, e, e / tw, tw))
        assert e <= 2 * max(tw, c["twin_all"])


def test_condition_gradient_stays_inside_its_sample_and_the_step_repeats(tiny_cfg):
    """dparams zero outside sample 1: d_pts_condition and d_img_condition are exactly 0 for samples 0 and 2 (a key loop, a batch stride or
    a per-sample row taken from the wrong sample would leak).  A second forward + backward repeats bit for bit."""
    c = ragged_case(tiny_cfg)
    mask = torch.zeros(RAGGED["B"], 1, 1, device="cuda")
    mask[1] = 1.0
    _, _, (d_pts, d_img) = ragged_step(c, mask)
    assert float(d_pts[[0, 2]].abs().max()) == 0.0 and float(d_img[[0, 2]].abs().max()) == 0.0
    assert float(d_pts[1].abs().max()) > 0.0 and float(d_img[1].abs().max()) > 0.0
    a, b = ragged_step(c), ragged_step(c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2][0], b[2][0]) and torch.equal(a[2][1], b[2][1])
    for n in c["names"]:
        assert torch.equal(a[1][n], b[1][n]), n


def test_too_many_tokens_are_refused_before_anything_is_kept(tiny_cfg):
    import ldt_amd.train as train
    model, x, t, _, _ = tt.make_case(tiny_cfg.score, 128, 2, 1, 1, 8, 1, None)
    model.cuda()
    tt.flat_grads(model)
    step = train.ScoreTrainStep(model, allow_condition=True)
    with pytest.raises(NotImplementedError, match=r"8 query and 520 condition tokens.*ldt_attention_bwd_cross"):
        step.forward(x.cuda(), t.cuda(), condition=(torch.zeros(1, 128, 520, device="cuda"), 0.))
    assert step.saved is None
    with pytest.raises(NotImplementedError, match="ViPC / point condition"):             # a step built without allow_condition refuses a pair
        train.ScoreTrainStep(model).forward(x.cuda(), t.cuda(), condition=(torch.zeros(1, 128, 8, device="cuda"), 0.))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ protocol
def _points(cfg, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(B, cfg.data.tr_max_sample_points, 3, generator=g)
    pts = pts - pts.mean(1, keepdim=True)
    return pts / pts.norm(dim=-1).amax(1)[:, None, None]


def test_update_protocol_and_a_frozen_condition_net(tiny_cfg):
    """A model built with cfg.score.condition=True and weight_decay = 0: `update(data, (pts_condition, img_condition))` advances itr and
    returns a 0-dim device tensor; after two calls every c_net parameter and its EMA are bit-equal to their initial values (zero gradient
    through Adam + EMA), while the Score's own parameters have moved."""
    import numpy as np
    import ldt_amd
    cfg = tc.set_train_options(copy.deepcopy(tiny_cfg), "x")
    cfg.score.condition = True
    assert cfg.opt.weight_decay == 0
    torch.manual_seed(21)
    score = ldt_amd.Score(cfg.score)
    comp = ldt_amd.Compressor(cfg.compressor)
    comp.init()
    tr = ldt_amd.CompletionTrainer(cfg, score, comp, "cuda")
    init = {n: p.detach().cpu().clone() for n, p in tr.model.named_parameters()}
    B, S = 3, 12
    g = torch.Generator().manual_seed(8)
    pair = (torch.randn(B, cfg.score.hidden_size, S, generator=g).cuda() * 0.5, torch.randn(B, cfg.score.t_dim, generator=g).cuda() * 0.5)
    data = _points(cfg, B)
    np.random.seed(5); torch.manual_seed(5)
    for i, d in enumerate((data, {"tr_points": data})):       # a tensor as upstream; a dict with tr_points is accepted too
        loss = tr.update(d, pair)
        assert tr.itr == i + 1 and loss.shape == () and loss.is_cuda and bool(torch.isfinite(loss))
        assert tr.last_condition_grad[0].shape == pair[0].shape and tr.last_condition_grad[1].shape == pair[1].shape
    frozen = [n for n in init if n.startswith("c_net.")]
    assert len(frozen) > 20
    for n, p in tr.model.named_parameters():
        ema = tr.optimizer.state[p]["ema"]
        if n.startswith("c_net."):
            assert torch.equal(p.detach().cpu(), init[n]) and torch.equal(ema.cpu(), init[n]), n
        elif p.numel() > 8:
            assert not torch.equal(p.detach().cpu(), init[n]), n
