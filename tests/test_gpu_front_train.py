"""GPU (-m gpu): one training step of the Compressor's front on the HIP path (ldt_amd/compressor_train.py: FrontTrainStep;
CompressorTrainer.update_front), whole.  The yardstick is test_gpu_decoder_train.py's (DESIGN.md sections 4.11 / 4.15): per tensor, rel-MSE
<= 2 x max(the bf16 twin's on that tensor, the twin's overall) — with one addition the front needs (section 4.19): it holds discrete
selections (three ReLUs and the max over the neighbours in the grouper, two ReLUs and the max over the tokens in MiniPointnet), a few of which
a correct bf16 forward makes differently from float64, and under free autograd those few cells dominate the error.  So the float64
restatement (tests/front_train_checks.py) and its twin are differentiated AT THE DEVICE'S SELECTIONS, and the share of cells on which the
device's forward and the float64 restatement select differently is held as a condition of its own.

Case `tiny`, against tests/golden/front_train_tiny.npz (tools/gen_front_train_golden.py: the reference's own input, group, pos_embedding,
conv_in, encoder and top_down in training mode under autograd; hidden 64, 8 tokens of k = 16 neighbours, N = 64, B = 3):
  * (1) forward: tokens and pos against the float64 restatement at 2 x the twin's rel-MSE; the four BatchNorms' buffers after one step
    against the fixture's
  * (2) selections: at most 2 % of arg-max cells and 1 % of ReLU cells per layer differ from the float64 restatement's
  * (3) backward: the front alone from the fixture's d_tokens / d_pos, then the chain front -> encoder -> top-down from ONE d_set: every
    gradient against the restatement at the device's selections; the analytically zero gradients (front_train_checks.FRONT_DEAD) against
    their live neighbours; a second forward + backward repeats bit for bit
  * (4) ten update_front steps against the fixture's trajectory, next to the twin's
  * (5) state: no parameter is left without a gradient, Compressor.forward afterwards runs on the new weights AND the new running
    statistics, update_encoder on a fresh trainer leaves the front bit-unchanged
Case `ragged`, FrontTrainStep alone: hidden 128, 24 tokens of k = 8, N = 96, B = 2, p_dim 40, norm_input on.

Before the step existed every test here ended at the missing `FrontTrainStep` or `update_front`."""
import copy
import os

import numpy as np
import pytest
import torch

import decoder_train_checks as dc
import encoder_train_checks as ec
import front_train_checks as fc
import topdown_train_checks as tc
from conftest import GOLDEN, rel_mse
from test_gpu_decoder_train import check_against_twin, digest, same_digest

pytestmark = pytest.mark.gpu
_CACHE = {}
TOL_DECODE = 1e-4                                                       # tests/test_gpu_path.py
ARG_CAP, RELU_CAP = 0.02, 0.01
# an analytically zero gradient on the device: what reaches it is the rounding of the bf16 GEMM operands (2^-8 per element, uncorrelated over
# the rows) against a live gradient summed over the same rows with O(1) weights
DEAD_CAP = 2.0 ** -6


def golden():
    if "g" not in _CACHE:
        z = np.load(os.path.join(GOLDEN, "front_train_tiny.npz"))
        _CACHE["g"] = {k: (torch.from_numpy(np.asarray(z[k])) if z[k].dtype.kind in "fiub" else z[k]) for k in z.files}
    return _CACHE["g"]


def train_cfg(tiny_cfg):
    g = golden()
    cfg = copy.deepcopy(tiny_cfg)
    cfg.opt.lr, cfg.opt.warmup_iters, cfg.opt.grad_norm_clip_value = float(g["lr"]), int(g["warmup_iters"]), float(g["grad_norm_clip_value"])
    cfg.opt.kl_weight = float(g["kl_weight"])
    return cfg


def tiny_model(cfg):
    import ldt_amd
    g = golden()
    torch.manual_seed(int(g["seed"]))
    model = ldt_amd.Compressor(cfg.compressor)
    model.init()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ec.perturb_actnorm(init)
    model.load_state_dict(init)
    for k, v in init.items():
        assert same_digest(digest(v), g["init_digest::" + k], v.numel()), "initial weights differ from the fixture's: " + k
    return model, init


def all_names(model):
    from ldt_amd.compressor_train import encoder_parameters, front_parameters, topdown_parameters
    return [n for n, _ in front_parameters(model)], [n for n, _ in encoder_parameters(model) + topdown_parameters(model)]


def device_front(model, cloud):
    """FrontTrainStep.forward -> (step, tokens, pos, the device's selections (CPU), fps_idx, knn_idx (CPU, int64))."""
    from ldt_amd import ops
    from ldt_amd.compressor_train import FrontTrainStep
    step = FrontTrainStep(model)
    tok, pos = step.forward(cloud.cuda())
    S, D = step.saved, model.hidden_dim
    a2 = ops.bn_relu_fwd(S["y2"], S["sp2"], S["gp2"], S["bp2"], out_bf16=False)                 # (the tape keeps its max alone)
    sel = {"mask1": S["h1"][:, :D] > 0, "mask2": S["r"][:, :D] > 0, "mask3": S["tok"] > 0, "arg": S["arg"], "pmask1": S["a1"] > 0, "pmask2": a2 > 0,
           "parg": S["argp"]}
    return step, tok, pos, {k: v.cpu() for k, v in sel.items()}, step.fps_idx.cpu().long(), step.knn_idx.cpu().long()


def front_grads(model):
    from ldt_amd.compressor_train import front_parameters
    return {n: p.grad.detach().clone() for n, p in front_parameters(model)}


def check_dead(got, what):
    for n, live in fc.FRONT_DEAD.items():
        r = float(got[n].abs().max()) / float(got[live].abs().max())
        print("%s %-45s analytically zero: max |grad| = %.2e x max |%s|" % (what, n, r, live))
        assert r <= DEAD_CAP, (n, r)


def live(d):
    return {n: v for n, v in d.items() if n not in fc.FRONT_DEAD}


def test_tiny_forward_selections_and_buffers(tiny_cfg):
    g = golden()
    cfg = train_cfg(tiny_cfg)
    c = cfg.compressor
    model, init = tiny_model(cfg)
    model = model.cuda().train()
    cloud = g["cloud"]
    step, tok, pos, dsel, fi, ki = device_front(model, cloud)
    B, T, D = cloud.shape[0], c.z_scales, c.hidden_dim
    assert tuple(tok.shape) == (B, T, D) and tuple(pos.shape) == (B, c.p_dim) and tok.dtype == torch.float32
    assert torch.equal(fi, g["fps_idx"].long()) and torch.equal(ki.sort(2).values, g["knn_idx"].long().sort(2).values)     # the same grouping, as sets
    # (1) the forward against the float64 restatement on the device's own (ordered) grouping
    _, t64, p64, sel64, bns = fc.front_step(init, c, cloud, fi, ki, g["d_tokens"], g["d_pos"], torch.float64)
    _, tt, pt, selt, bnst = fc.front_step(init, c, cloud, fi, ki, g["d_tokens"], g["d_pos"], torch.float32, twin=True)
    assert rel_mse(t64, g["tokens"]) < 1e-12 and rel_mse(p64, g["pos"]) < 1e-12                                             # the fixture's leaves
    e_tok, e_pos, t_tok, t_pos = rel_mse(tok.cpu(), t64), rel_mse(pos.cpu(), p64), rel_mse(tt, t64), rel_mse(pt, p64)
    print("tiny forward: tokens rel-MSE %.3e = %.2f x the twin's %.3e; pos rel-MSE %.3e (twin %.3e: fp32 on both sides)" % (e_tok, e_tok / t_tok, t_tok, e_pos, t_pos))
    assert e_tok <= 2 * t_tok and e_pos <= max(2 * t_pos, 1e-12)
    # the BatchNorm buffers after ONE step, against the fixture's and against the restatement's
    want, twin_after = fc.running_after(init, bns), fc.running_after(init, bnst)
    now = model.state_dict()
    for k, w in want.items():
        got = now[k].detach().cpu()
        if k.endswith("num_batches_tracked"):
            assert int(got) == 1 and int(g["bn::" + k]) == 1
            continue
        e, t = rel_mse(got, w), rel_mse(twin_after[k], w)
        print("tiny buffers %-55s rel-MSE %.3e  twin %.3e  vs the fixture %.3e" % (k, e, t, rel_mse(got, g["bn::" + k])))
        assert e <= max(2 * t, 1e-12) and rel_mse(g["bn::" + k], w) < 1e-12 and not torch.equal(got, init[k])
    # (2) the selections
    shares, tshares = fc.selection_shares(dsel, sel64), fc.selection_shares(selt, sel64)
    print("tiny selections, share of cells that differ from float64: " + "  ".join("%s %.4f (twin %.4f)" % (k, shares[k], tshares[k]) for k in shares))
    assert max(shares["arg"], shares["parg"]) <= ARG_CAP and max(shares[k] for k in ("mask1", "mask2", "mask3", "pmask1", "pmask2")) <= RELU_CAP
    # the packed panels were dropped: the evaluation path folds the new buffers
    assert model._pack is None


def test_tiny_front_alone_at_the_devices_selections(tiny_cfg):
    g = golden()
    cfg = train_cfg(tiny_cfg)
    c = cfg.compressor
    model, init = tiny_model(cfg)
    model = model.cuda().train()
    cloud, d_tok, d_pos = g["cloud"], g["d_tokens"], g["d_pos"]

    def run():
        step, tok, pos, dsel, fi, ki = device_front(model, cloud)
        step.backward(d_tok.cuda(), d_pos.cuda())
        assert step.saved is None
        return front_grads(model), tok.clone(), pos.clone(), dsel, fi, ki

    got, tok, pos, dsel, fi, ki = run()
    ref, _, _, rsel, _ = fc.front_step(init, c, cloud, fi, ki, d_tok, d_pos, torch.float64, sel=dsel)
    twin, _, _, _, _ = fc.front_step(init, c, cloud, fi, ki, d_tok, d_pos, torch.float32, sel=dsel, twin=True)
    assert all(torch.equal(rsel[k].to(dsel[k].dtype), dsel[k]) for k in fc.FRONT_SELECTIONS)
    free, _, _, _, _ = fc.front_step(init, c, cloud, fi, ki, d_tok, d_pos, torch.float64)
    stored = [n for n in fc.front_names(init) if "grad::" + n in g and n not in fc.FRONT_DEAD]
    assert len(stored) >= 10                                           # the fixture's gradients are the restatement's under FREE autograd
    assert all(rel_mse(free[n], g["grad::" + n]) <= 1e-9 for n in stored)
    check_against_twin(live(got), live(ref), live(twin), "tiny (3a) front alone")
    cat = lambda d: torch.cat([d[n].double().cpu().reshape(-1) for n in live(ref)])
    print("tiny (3a) against FREE float64 autograd instead: all tensors rel-MSE %.3e (at the device's selections %.3e)" % (rel_mse(cat(got), cat(free)), rel_mse(cat(got), cat(ref))))
    check_dead(got, "tiny (3a)")
    named = dict(model.named_parameters())
    assert all(p.grad is None for n, p in named.items() if n not in got)
    got2, tok2, pos2, dsel2, _, _ = run()                                # fixed order everywhere: the same bits
    assert torch.equal(tok2, tok) and torch.equal(pos2, pos) and all(torch.equal(got2[n], got[n]) for n in got)
    assert all(torch.equal(dsel2[k], dsel[k]) for k in dsel)
    assert int(model.pos_embedding.bn1.num_batches_tracked) == 2


def test_tiny_chain_from_one_d_set(tiny_cfg):
    from ldt_amd.compressor_train import EncoderTrainStep, TopDownTrainStep
    g = golden()
    cfg = train_cfg(tiny_cfg)
    c, kw = cfg.compressor, float(g["kl_weight"])
    model, init = tiny_model(cfg)
    fr_names, rest = all_names(model)
    assert fr_names == [str(n) for n in g["front_names"]]
    names = fr_names + rest
    assert sorted(names) == sorted(n for n, _ in model.named_parameters())
    L = c.n_layers
    cloud, target = g["cloud"], g["target"]
    post_noise = [g["post_noise.%d" % i] for i in range(L)]
    B = target.shape[0]
    n_kl = L * B * c.z_dim * c.z_scales
    model = model.cuda().train()
    step, tok, pos, dsel, fi, ki = device_front(model, cloud)
    ref, ref_loss, _, _, _, _ = fc.whole_step(init, c, names, cloud, fi, ki, post_noise, target, torch.float64, kw, sel=dsel)
    assert abs(ref_loss[0] - float(g["loss"])) <= 1e-3 * abs(float(g["loss"]))            # (the device's selections move the loss a little)
    twin = fc.whole_step(init, c, names, cloud, fi, ki, post_noise, target, torch.float32, kw, sel=dsel, twin=True, d_set=ref["d_set"])[0]
    enc, top = EncoderTrainStep(model), TopDownTrainStep(model)
    outs = enc.forward(tok, pos)
    pts, _, kls = top.forward(outs, [t.cuda() for t in post_noise])
    d_tokens, d_pos = enc.backward(top.backward(ref["d_set"].float().cuda(), kw / n_kl))
    step.backward(d_tokens, d_pos)
    got = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    got["d_tokens"], got["d_pos"] = d_tokens.clone(), d_pos.clone()
    assert all(v is not None for v in got.values())
    print("tiny chain: set rel-MSE %.2e vs the fixture's" % rel_mse(pts.cpu(), g["set"]))
    drop = lambda d: {n: v for n, v in d.items() if n not in fc.FRONT_DEAD and n != "d_set"}
    check_against_twin(drop(got), drop(ref), drop(twin), "tiny (3b) chain from one d_set")
    check_dead(got, "tiny (3b)")


def twin_trajectory(cfg, init, names, cloud, fi, ki, post_noise, target, kw, ref):
    """The bf16 twin's ten steps: whole_step(twin) + clip + Adam on the same batch -> its losses."""
    sd = {k: v.detach().clone() for k, v in init.items()}
    params = [sd[n] for n in names]
    opt = torch.optim.Adam([p.requires_grad_(True) for p in params], lr=cfg.opt.lr, betas=(cfg.opt.beta1, cfg.opt.beta2), weight_decay=cfg.opt.weight_decay)
    out = []
    for i in range(len(ref)):
        if i < cfg.opt.warmup_iters:
            for grp in opt.param_groups:
                grp["lr"] = cfg.opt.lr * min(float(i + 1) / max(cfg.opt.warmup_iters, 1), 1.0)
        grads, losses, _, _, _, _ = fc.whole_step({k: v.detach() for k, v in sd.items()}, cfg.compressor, names, cloud, fi, ki, post_noise, target,
                                                  torch.float32, kw, twin=True)
        for p, n in zip(params, names):
            p.grad = grads[n].float()
        torch.nn.utils.clip_grad_norm_(params, cfg.opt.grad_norm_clip_value)
        opt.step()
        out.append(losses[0])
    return out


def test_tiny_ten_steps_of_update_front_and_the_state_after(tiny_cfg):
    import ldt_amd
    from oracle import ldt_oracle as O
    g = golden()
    cfg = train_cfg(tiny_cfg)
    c, kw = cfg.compressor, float(g["kl_weight"])
    model, init = tiny_model(cfg)
    fr_names, rest = all_names(model)
    names = fr_names + rest
    L = c.n_layers
    cloud, target = g["cloud"], g["target"]
    post_noise = [g["post_noise.%d" % i] for i in range(L)]
    ref = g["traj_loss"].tolist()
    twin = twin_trajectory(cfg, init, names, cloud, g["fps_idx"].long(), g["knn_idx"].long(), post_noise, target, kw, ref)
    # the loss crosses zero on this trajectory (0.42 -> -0.13: the KL estimate goes negative), so a deviation relative to the loss itself is
    # unbounded near the crossing: both sides are measured against the FIRST loss, the scale of the trajectory
    scale = abs(ref[0])
    twin_dev = max(abs(a - b) for a, b in zip(twin, ref)) / scale
    tr = ldt_amd.CompressorTrainer(cfg, model, "cuda")
    assert tr.front_optimizer is None
    model.train()
    nz_d = [t.cuda() for t in post_noise]
    losses = []
    for i in range(len(ref)):
        loss, kl_loss, rec_loss = tr.update_front({"tr_points": target}, post_noise=nz_d)
        assert loss.dim() == 0 and loss.is_cuda and abs(float(loss) - (kw * float(kl_loss) + float(rec_loss))) <= 1e-6 * abs(float(loss)) + 1e-7
        losses.append(float(loss))
    dev = max(abs(a - b) for a, b in zip(losses, ref)) / scale
    print("tiny 10-step trajectory: %.4f -> %.4f (reference %.4f -> %.4f, twin -> %.4f); worst deviation / |first loss| %.3e = %.2f x the twin's %.3e"
          % (losses[0], losses[-1], ref[0], ref[-1], twin[-1], dev, dev / twin_dev, twin_dev))
    assert min(ref) < 0 < max(ref)                                       # the crossing the measure above is chosen for
    assert dev <= 2 * twin_dev
    assert losses[-1] < losses[0] and model.training
    assert tr.itr == len(ref) and isinstance(tr.front_optimizer, ldt_amd.AdamEMA) and not tr.front_optimizer.apply_ema
    assert tr.encoder_optimizer is None and tr.topdown_optimizer is None and tr.optimizer is None
    # (5) every parameter has a gradient and has moved; the buffers were updated ten times
    named = dict(model.named_parameters())
    assert all(p.grad is not None for p in named.values())
    assert all(not torch.equal(named[n].detach().cpu(), init[n]) for n in names if named[n].numel() > 1 and n not in fc.FRONT_DEAD)
    assert all(int(b.num_batches_tracked) == len(ref) for b in (model.pos_embedding.bn1, model.pos_embedding.bn2))
    # Compressor.forward afterwards runs on the new weights AND the new running statistics (the eval path folds them)
    now = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    want = O.compressor_encode(now, c, cloud, post_noise)
    model.eval()
    fwd = model(cloud.cuda(), post_noise=nz_d)
    assert rel_mse(fwd["set"].cpu(), want["set"]) < TOL_DECODE and rel_mse(fwd["all_eps"].cpu(), want["all_eps"]) < TOL_DECODE
    stale = dict(now)
    stale.update({k: init[k] for k in init if "running_" in k})
    old = O.compressor_encode(stale, c, cloud, post_noise)
    assert rel_mse(fwd["all_eps"].cpu(), old["all_eps"]) > 100 * TOL_DECODE                  # the stale buffers would show


def test_update_encoder_still_leaves_the_front_bit_unchanged(tiny_cfg):
    import ldt_amd
    g = golden()
    cfg = train_cfg(tiny_cfg)
    model, init = tiny_model(cfg)
    tr = ldt_amd.CompressorTrainer(cfg, model, "cuda")
    model.train()
    tr.update_encoder({"tr_points": g["cloud"]}, post_noise=[g["post_noise.%d" % i].cuda() for i in range(cfg.compressor.n_layers)])
    now = model.state_dict()
    for k, v in init.items():
        if k.split(".")[0] in ("input", "group", "pos_embedding"):
            assert torch.equal(now[k].cpu(), v), k                       # parameters and BatchNorm buffers alike
    assert all(p.grad is None for n, p in model.named_parameters() if n.split(".")[0] in ("input", "group", "pos_embedding")) and model.training


def test_ragged_front_against_the_float64_restatement(tiny_cfg):
    import ldt_amd
    c = copy.deepcopy(tiny_cfg.compressor)
    c.hidden_dim, c.num_heads, c.n_layers, c.encoder_layers, c.p_dim, c.z_scales, c.outsize, c.max_outputs, c.norm_input = 128, 4, 2, 1, 40, 24, 96, 96, True
    B = 2
    torch.manual_seed(8)
    model = ldt_amd.Compressor(c)
    model.init()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(12)
    cloud = torch.randn(B, c.outsize, 3, generator=gen) * torch.tensor([0.5, 1.0, 2.0]) + 0.3
    d_tok = torch.randn(B, c.z_scales, c.hidden_dim, generator=gen) * 0.05
    d_pos = torch.randn(B, c.p_dim, generator=gen) * 0.05
    model = model.cuda().train()
    step, tok, pos, dsel, fi, ki = device_front(model, cloud)
    assert ki.shape[2] == 8 and step.saved["U"].shape[0] == B * 24 * 8
    step.backward(d_tok.cuda(), d_pos.cuda())
    got = front_grads(model)
    normed = (cloud.double() - cloud.double().mean(1, keepdim=True)) / cloud.double().std(1, keepdim=True)                  # norm_pts: a transform of data
    ref, t64, p64, _, _ = fc.front_step(init, c, normed, fi, ki, d_tok, d_pos, torch.float64, sel=dsel)
    twin, tt, pt, _, _ = fc.front_step(init, c, normed, fi, ki, d_tok, d_pos, torch.float32, sel=dsel, twin=True)
    _, f64, p64f, sel64, _ = fc.front_step(init, c, normed, fi, ki, d_tok, d_pos, torch.float64)
    _, tf, ptf, _, _ = fc.front_step(init, c, normed, fi, ki, d_tok, d_pos, torch.float32, twin=True)                      # the twin at its OWN selections
    shares = fc.selection_shares(dsel, sel64)
    print("ragged selections, share of cells that differ from float64: " + "  ".join("%s %.4f" % kv for kv in shares.items()))
    assert max(shares["arg"], shares["parg"]) <= ARG_CAP and max(shares[k] for k in ("mask1", "mask2", "mask3", "pmask1", "pmask2")) <= RELU_CAP
    e, t = rel_mse(tok.cpu(), f64), rel_mse(tf, f64)                                                                       # both free, as the tiny case
    e_pos, t_pos = rel_mse(pos.cpu(), p64f), rel_mse(ptf, p64f)
    print("ragged forward: tokens rel-MSE %.3e = %.2f x the twin's %.3e against free float64; pos %.3e (twin %.3e: fp32 on both sides)" % (e, e / t, t, e_pos, t_pos))
    assert e <= 2 * t and e_pos <= max(2 * t_pos, 1e-12)
    check_against_twin(live(got), live(ref), live(twin), "ragged front")
    check_dead(got, "ragged")
