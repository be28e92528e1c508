"""GPU (-m gpu): one training step of the Compressor's encoder on the HIP path (ldt_amd/compressor_train.py: EncoderTrainStep;
CompressorTrainer.update_encoder; Compressor.front), whole.  The yardstick is the one of test_gpu_decoder_train.py (DESIGN.md sections
4.11 / 4.15): per tensor, rel-MSE <= 2 x max(the bf16 twin's on that tensor, the twin's overall), the twin being the float64 restatement
(tests/encoder_train_checks.py, from the oracle's pieces) under torch.autocast("cpu", bfloat16).

Case `tiny`, against tests/golden/encoder_train_tiny.npz (tools/gen_encoder_train_golden.py: the reference's own conv_in, encoder[i] and
top_down under autograd; hidden 64, 2 heads of 32, 3 stages x 2 blocks, 8 tokens, p_dim 32, B = 3; ActNorm perturbed away from the identity):
  * the stage outputs at the decode bar (rel-MSE 1e-4) against Compressor.bottom_up on the same weights, and against the fixture's
  * (1) the encoder alone from the fixture's d_enc_out: every encoder gradient, d_tokens and d_pos within the yardstick
  * (2) the chain encoder -> top-down from ONE d_set, the reference's, with the KL path on: both parameter lists
  * (3) d_enc_out = 0 for all but the LAST stage, then all but the FIRST: conv_in.* and stage 0's gradients still within the yardstick
    (the chain accumulation: a backward that drops the running dX fails here)
  * (4) 10 update_encoder steps on one batch: the loss falls, its worst relative deviation from the reference trajectory <= 2 x the
    twin's, every frozen parameter bit-unchanged with .grad None, Compressor.forward afterwards runs on the NEW weights
  * (5) with `initialized` = 0 the first update_encoder sets shift / log_scale to the batch statistics of front's tokens; a second
    step does not re-initialise
Case `ragged`, EncoderTrainStep alone against the float64 restatement, each run from its own start with seeded d_enc_out: hidden 128, 4
heads, 2 stages x 2 blocks, p_dim 40, 24 tokens (a partial 16-row tile), B = 2, ActNorm perturbed; once more with `ActNorm: ~`.
A second forward + backward repeats bit for bit, d_tokens and d_pos included.

Before the step existed every test here ended at the missing `EncoderTrainStep`, `update_encoder` or `front`."""
import copy
import os

import numpy as np
import pytest
import torch

import decoder_train_checks as dc
import encoder_train_checks as ec
import topdown_train_checks as tc
from conftest import GOLDEN, rel_mse
from test_gpu_decoder_train import check_against_twin, digest, same_digest

pytestmark = pytest.mark.gpu
_CACHE = {}
TOL_DECODE = 1e-4                                                       # tests/test_gpu_path.py


def golden():
    if "g" not in _CACHE:
        z = np.load(os.path.join(GOLDEN, "encoder_train_tiny.npz"))
        _CACHE["g"] = {k: (torch.from_numpy(np.asarray(z[k])) if z[k].dtype.kind in "fiu" else z[k]) for k in z.files}
    return _CACHE["g"]


def train_cfg(tiny_cfg):
    g = golden()
    cfg = copy.deepcopy(tiny_cfg)
    cfg.opt.lr, cfg.opt.warmup_iters, cfg.opt.grad_norm_clip_value = float(g["lr"]), int(g["warmup_iters"]), float(g["grad_norm_clip_value"])
    cfg.opt.kl_weight = float(g["kl_weight"])
    return cfg


def tiny_model(cfg):
    """The fixture's initial Compressor (rebuilt from its seed, ActNorm overwritten as the fixture's, checked against the digests)
    -> (model on the CPU, its state_dict copy)."""
    import ldt_amd
    g = golden()
    torch.manual_seed(int(g["seed"]))
    model = ldt_amd.Compressor(cfg.compressor)
    model.init()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ec.perturb_actnorm(init)
    assert torch.equal(init["conv_in.shift"], g["actnorm_shift"]) and torch.equal(init["conv_in.log_scale"], g["actnorm_log_scale"])
    model.load_state_dict(init)
    for k, v in init.items():
        assert same_digest(digest(v), g["init_digest::" + k], v.numel()), "initial weights differ from the fixture's: " + k
    return model, init


def names_of(model):
    from ldt_amd.compressor_train import encoder_parameters, topdown_parameters
    return [n for n, _ in encoder_parameters(model)], [n for n, _ in topdown_parameters(model)]


def hip_encoder(model, tokens, pos, d_enc_out):
    """EncoderTrainStep forward + backward -> ({name: grad, 'd_tokens', 'd_pos'}, the stage outputs)."""
    from ldt_amd.compressor_train import EncoderTrainStep, encoder_parameters
    step = EncoderTrainStep(model)
    outs = step.forward(tokens.cuda(), pos.cuda())
    d_tokens, d_pos = step.backward([t.float().cuda() for t in d_enc_out])
    assert d_tokens is step.d_tokens and d_pos is step.d_pos and step.saved is None
    got = {n: p.grad.detach().clone() for n, p in encoder_parameters(model)}
    got["d_tokens"], got["d_pos"] = d_tokens.clone(), d_pos.clone()
    return got, [o.clone() for o in outs]


def test_tiny_stage_outputs_against_bottom_up_and_the_fixture(tiny_cfg):
    from ldt_amd.compressor_train import EncoderTrainStep
    g = golden()
    cfg = train_cfg(tiny_cfg)
    c = cfg.compressor
    model, _ = tiny_model(cfg)
    model = model.cuda().eval()
    cloud = g["cloud"].cuda()
    B, T, C = cloud.shape[0], c.z_scales, c.hidden_dim
    fr = model.front(cloud)
    assert sorted(fr) == ["centers", "fps_idx", "knn_idx", "pos", "tokens"]
    assert tuple(fr["tokens"].shape) == (B, T, C) and tuple(fr["pos"].shape) == (B, c.p_dim) and fr["tokens"].dtype == torch.float32
    bup = model.bottom_up(cloud)
    assert torch.equal(fr["fps_idx"], bup["fps_idx"]) and torch.equal(fr["knn_idx"], bup["knn_idx"]) and torch.equal(fr["centers"], bup["centers"])
    print("tiny front vs the oracle's pieces: tokens rel-MSE %.2e, pos rel-MSE %.2e" % (rel_mse(fr["tokens"].cpu(), g["tokens"]), rel_mse(fr["pos"].cpu(), g["pos"])))
    assert rel_mse(fr["tokens"].cpu(), g["tokens"]) < TOL_DECODE and rel_mse(fr["pos"].cpu(), g["pos"]) < TOL_DECODE
    step = EncoderTrainStep(model)
    outs = step.forward(fr["tokens"], fr["pos"])
    assert len(outs) == c.n_layers
    for i, (o, b) in enumerate(zip(outs, bup["outputs"])):
        e = rel_mse(o, b.transpose(1, 2))
        print("tiny stage %d: the step's unfused forward vs Compressor.bottom_up rel-MSE %.2e; vs the fixture's %.2e" % (i, e, rel_mse(o.cpu(), g["enc_out.%d" % i])))
        assert tuple(o.shape) == (B, T, C) and o.is_contiguous() and e < TOL_DECODE
    # on the fixture's own leaves, against the reference's stage outputs
    outs = EncoderTrainStep(model).forward(g["tokens"].cuda(), g["pos"].cuda())
    for i, o in enumerate(outs):
        assert rel_mse(o.cpu(), g["enc_out.%d" % i]) < TOL_DECODE, i
    assert len({o.data_ptr() for o in outs}) == c.n_layers                                   # fresh buffers


def test_tiny_encoder_alone_and_the_stage_chain(tiny_cfg):
    g = golden()
    cfg = train_cfg(tiny_cfg)
    c = cfg.compressor
    model, init = tiny_model(cfg)
    enc_names, _ = names_of(model)
    assert enc_names == [str(n) for n in g["encoder_names"]]
    L = c.n_layers
    tokens, pos = g["tokens"], g["pos"]
    d_enc = [g["d_enc_out.%d" % i] for i in range(L)]
    model = model.cuda()
    # (1) the encoder alone, from the fixture's d_enc_out
    ref, _ = ec.encoder_step(init, c, enc_names, tokens, pos, d_enc, torch.float64)
    for k in ("d_tokens", "d_pos"):
        assert rel_mse(ref[k], g[k]) <= 1e-9
    twin, _ = ec.encoder_step(init, c, enc_names, tokens, pos, d_enc, torch.float32, autocast=True)
    got, outs = hip_encoder(model, tokens, pos, d_enc)
    check_against_twin(got, ref, twin, "tiny (1) encoder alone")
    assert tuple(got["d_tokens"].shape) == tuple(tokens.shape) and tuple(got["d_pos"].shape) == tuple(pos.shape)
    named = dict(model.named_parameters())
    assert all(p.grad is None for n, p in named.items() if n not in enc_names)
    got2, outs2 = hip_encoder(model, tokens, pos, d_enc)                                     # fixed order everywhere: the same bits
    assert all(torch.equal(a, b) for a, b in zip(outs2, outs)) and all(torch.equal(got2[n], got[n]) for n in got)
    # (3) the chain accumulation: only the LAST stage's output has a gradient, then only the FIRST's
    held = [n for n in enc_names if n.startswith(("conv_in.", "encoder.0."))] + ["d_tokens", "d_pos"]
    for keep, what in ((L - 1, "last"), (0, "first")):
        d_one = [d if i == keep else torch.zeros_like(d) for i, d in enumerate(d_enc)]
        ref1, _ = ec.encoder_step(init, c, enc_names, tokens, pos, d_one, torch.float64)
        twin1, _ = ec.encoder_step(init, c, enc_names, tokens, pos, d_one, torch.float32, autocast=True)
        got1, _ = hip_encoder(model, tokens, pos, d_one)
        # (stage 0's own conv_out feeds nothing when only the last stage's output has a gradient: exactly 0 on both sides)
        dead = [n for n in held if n.startswith("encoder.0.conv_out.")] if keep else []
        assert all(float(ref1[n].abs().max()) > 0 for n in held if n not in dead)
        assert all(bool((got1[n] == 0).all()) and bool((ref1[n] == 0).all()) for n in dead)
        check_against_twin({n: got1[n] for n in held}, {n: ref1[n] for n in held}, {n: twin1[n] for n in held},
                           "tiny (3) d_enc_out of the %s stage alone" % what)
        if keep == 0:                                                                        # nothing flows back from a later stage
            later = [n for n in enc_names if n.startswith(("encoder.1.", "encoder.2."))]
            assert all(bool((got1[n] == 0).all()) and bool((ref1[n] == 0).all()) for n in later)


def test_tiny_chain_from_one_d_set(tiny_cfg):
    from ldt_amd.compressor_train import EncoderTrainStep, TopDownTrainStep, encoder_parameters, topdown_parameters
    g = golden()
    cfg = train_cfg(tiny_cfg)
    c, kw = cfg.compressor, float(g["kl_weight"])
    model, init = tiny_model(cfg)
    enc_names, top_names = names_of(model)
    names = enc_names + top_names
    assert top_names == [str(n) for n in g["topdown_names"]]
    L = c.n_layers
    tokens, pos, target = g["tokens"], g["pos"], g["target"]
    post_noise = [g["post_noise.%d" % i] for i in range(L)]
    B = target.shape[0]
    n_kl = L * B * c.z_dim * c.z_scales
    ref, ref_loss, ref_set, _, _ = ec.chain_step(init, c, names, tokens, pos, post_noise, target, torch.float64, kw)
    assert abs(ref_loss[0] - float(g["loss"])) <= 1e-6 * abs(float(g["loss"])) and rel_mse(ref_set, g["set"]) < 1e-10
    twin = ec.chain_step(init, c, names, tokens, pos, post_noise, target, torch.float32, kw, autocast=True, d_set=ref["d_set"])[0]
    model = model.cuda()

    def run():
        enc, top = EncoderTrainStep(model), TopDownTrainStep(model)
        outs = enc.forward(tokens.cuda(), pos.cuda())
        pts, all_eps, kls = top.forward(outs, [t.cuda() for t in post_noise])
        d_enc = top.backward(ref["d_set"].float().cuda(), kw / n_kl)
        d_tokens, d_pos = enc.backward(d_enc)
        got = {n: p.grad.detach().clone() for n, p in encoder_parameters(model) + topdown_parameters(model)}
        got.update({"d_enc_out.%d" % i: t.clone() for i, t in enumerate(d_enc)})
        got["d_tokens"], got["d_pos"] = d_tokens.clone(), d_pos.clone()
        return got, pts, kls

    got, pts, kls = run()
    kl_loss = float(kls.sum()) / n_kl
    print("tiny chain: set rel-MSE %.2e; kl_loss %.6f vs %.6f (rel %.2e)" % (rel_mse(pts.cpu(), g["set"]), kl_loss, float(g["kl_loss"]),
                                                                               abs(kl_loss - float(g["kl_loss"])) / abs(float(g["kl_loss"]))))
    assert rel_mse(pts.cpu(), g["set"]) < TOL_DECODE and abs(kl_loss - float(g["kl_loss"])) <= 1e-3 * abs(float(g["kl_loss"]))
    check_against_twin(got, ref, twin, "tiny (2) chain from one d_set")
    named = dict(model.named_parameters())
    assert all(p.grad is None for n, p in named.items() if n not in names)
    got2, pts2, _ = run()
    assert torch.equal(pts2, pts) and all(torch.equal(got2[n], got[n]) for n in got)


def test_tiny_ten_steps_of_update_encoder(tiny_cfg):
    import ldt_amd
    from oracle import ldt_oracle as O
    g = golden()
    cfg = train_cfg(tiny_cfg)
    c, kw = cfg.compressor, float(g["kl_weight"])
    model, init = tiny_model(cfg)
    enc_names, top_names = names_of(model)
    names = enc_names + top_names
    L = c.n_layers
    tokens, pos, target = g["tokens"], g["pos"], g["target"]
    post_noise = [g["post_noise.%d" % i] for i in range(L)]
    ref = g["traj_loss"].tolist()
    # the bf16 twin's trajectory: autocast + autograd + clip + Adam on the same batch
    sd = {k: v.detach().clone() for k, v in init.items()}
    leaves = [sd[n].requires_grad_(True) for n in names]
    opt = torch.optim.Adam(leaves, lr=cfg.opt.lr, betas=(cfg.opt.beta1, cfg.opt.beta2), weight_decay=cfg.opt.weight_decay)
    twin_dev = 0.0
    for i in range(len(ref)):
        if i < cfg.opt.warmup_iters:
            for grp in opt.param_groups:
                grp["lr"] = cfg.opt.lr * min(float(i + 1) / max(cfg.opt.warmup_iters, 1), 1.0)
        opt.zero_grad()
        with torch.autocast("cpu", torch.bfloat16):
            pts, _, kls = tc.top_down(sd, c, ec.encoder(sd, c, tokens, pos), post_noise)
        loss = kw * torch.cat([k.float() for k in kls], dim=1).mean() + dc.cd_loss_torch(pts.float(), target, "l1")
        loss.backward()
        torch.nn.utils.clip_grad_norm_(leaves, cfg.opt.grad_norm_clip_value)
        opt.step()
        twin_dev = max(twin_dev, abs(float(loss.detach()) - ref[i]) / abs(ref[i]))
    tr = ldt_amd.CompressorTrainer(cfg, model, "cuda")
    assert tr.encoder_optimizer is None and tr.topdown_optimizer is None and tr.optimizer is None     # nothing allocated before the first call
    frozen = {n: p.detach().clone() for n, p in model.named_parameters() if n not in names}
    assert frozen and all(n.startswith(("input.", "group.", "pos_embedding.")) for n in frozen)
    tk_d, ps_d, nz_d = tokens.cuda(), pos.cuda(), [t.cuda() for t in post_noise]
    losses = []
    for i in range(len(ref)):
        loss, kl_loss, rec_loss = tr.update_encoder({"tr_points": target}, tokens=tk_d, pos=ps_d, post_noise=nz_d)
        assert loss.dim() == 0 and loss.is_cuda and kl_loss.dim() == 0 and rec_loss.dim() == 0
        assert abs(float(loss) - (kw * float(kl_loss) + float(rec_loss))) <= 1e-6 * abs(float(loss)) + 1e-7
        losses.append(float(loss))
    dev = max(abs(a - b) / abs(b) for a, b in zip(losses, ref))
    print("tiny 10-step trajectory: %.4f -> %.4f (reference %.4f -> %.4f); worst relative deviation %.3e = %.2f x the twin's %.3e"
          % (losses[0], losses[-1], ref[0], ref[-1], dev, dev / twin_dev, twin_dev))
    assert dev <= 2 * twin_dev
    assert losses[-1] < losses[0]
    assert tr.itr == len(ref) and isinstance(tr.encoder_optimizer, ldt_amd.AdamEMA) and not tr.encoder_optimizer.apply_ema
    assert tr.topdown_optimizer is None and tr.optimizer is None
    assert tuple(tr.last_tokens_grad.shape) == tuple(tokens.shape) and tuple(tr.last_pos_grad.shape) == tuple(pos.shape)
    assert bool(tr.last_tokens_grad.isfinite().all()) and bool(tr.last_pos_grad.isfinite().all())
    named = dict(model.named_parameters())
    for n, v in frozen.items():
        assert torch.equal(named[n].detach(), v) and named[n].grad is None, n
    assert all(not torch.equal(named[n].detach().cpu(), init[n]) for n in names if named[n].numel() > 1)
    assert float(model.conv_in.initialized) == 1                         # it was initialised: no data-dependent init ran
    # Compressor.forward runs on the weights the optimizer wrote through raw pointers
    now = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    want = O.compressor_encode(now, c, g["cloud"], post_noise)
    model.eval()
    fwd = model(g["cloud"].cuda(), post_noise=nz_d)
    assert rel_mse(fwd["set"].cpu(), want["set"]) < TOL_DECODE and rel_mse(fwd["set"].cpu(), g["set"]) > 100 * TOL_DECODE
    assert rel_mse(fwd["all_eps"].cpu(), want["all_eps"]) < TOL_DECODE
    # without `tokens` / `pos` / `post_noise` the step runs front itself, under no_grad and in evaluation mode, and hands the caller's mode back
    model.train()
    loss, kl_loss, rec_loss = tr.update_encoder({"tr_points": g["cloud"]})
    assert model.training and bool(loss.isfinite()) and tr.itr == len(ref) + 1
    for n, v in frozen.items():
        assert torch.equal(dict(model.named_parameters())[n].detach(), v), n


def test_tiny_data_dependent_actnorm_init(tiny_cfg):
    """lr = 0: the optimizer leaves every parameter where it is, so what the first step wrote into ActNorm can be read back."""
    import ldt_amd
    g = golden()
    cfg = train_cfg(tiny_cfg)
    cfg.opt.lr = 0.0
    model, init = tiny_model(cfg)
    with torch.no_grad():
        model.conv_in.initialized.zero_()
    tr = ldt_amd.CompressorTrainer(cfg, model, "cuda")
    cloud = g["cloud"]
    model.eval()
    tokens = model.front(cloud.cuda())["tokens"].cpu()
    model.train()
    post_noise = [g["post_noise.%d" % i].cuda() for i in range(cfg.compressor.n_layers)]
    loss, _, _ = tr.update_encoder({"tr_points": cloud}, post_noise=post_noise)
    assert bool(loss.isfinite()) and float(model.conv_in.initialized) == 1 and model.training
    shift, ls = model.conv_in.shift.detach().cpu(), model.conv_in.log_scale.detach().cpu()
    want_shift = torch.mean(tokens, dim=0, keepdim=True)
    want_ls = torch.log(torch.std(tokens, dim=0, keepdim=True) + model.conv_in.eps)
    print("data-dependent init: shift max |err| %.2e, log_scale max |err| %.2e" % (float((shift - want_shift).abs().max()), float((ls - want_ls).abs().max())))
    assert tuple(shift.shape) == tuple(want_shift.shape) and float((shift - want_shift).abs().max()) <= 1e-6
    assert float((ls - want_ls).abs().max()) <= 1e-6
    assert not torch.equal(shift, init["conv_in.shift"])
    # a second step, on another batch, does not re-initialise
    other = cloud.flip(0) * 0.9
    tr.update_encoder({"tr_points": other}, post_noise=post_noise)
    assert torch.equal(model.conv_in.shift.detach().cpu(), shift) and torch.equal(model.conv_in.log_scale.detach().cpu(), ls)
    assert float(model.conv_in.initialized) == 1 and tr.itr == 2


@pytest.mark.parametrize("actnorm", [True, None])
def test_ragged_encoder_against_the_float64_restatement(tiny_cfg, actnorm):
    import ldt_amd
    c = copy.deepcopy(tiny_cfg.compressor)
    c.hidden_dim, c.num_heads, c.n_layers, c.encoder_layers, c.p_dim, c.z_scales, c.ActNorm = 128, 4, 2, 2, 40, 24, actnorm
    B = 2
    torch.manual_seed(6)
    model = ldt_amd.Compressor(c)
    model.init()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if actnorm is not None:
        ec.perturb_actnorm(init, seed=78)
        model.load_state_dict(init)
    enc_names, _ = names_of(model)
    assert ("conv_in.shift" in enc_names) == (actnorm is not None)
    g = torch.Generator().manual_seed(10)
    tokens = torch.randn(B, c.z_scales, c.hidden_dim, generator=g) * 1.3 + 0.2
    pos = torch.randn(B, c.p_dim, generator=g)
    d_enc = [torch.randn(B, c.z_scales, c.hidden_dim, generator=g) * 0.05 for _ in range(c.n_layers)]
    what = "ragged" if actnorm is not None else "ragged, ActNorm: ~"
    ref, ref_out = ec.encoder_step(init, c, enc_names, tokens, pos, d_enc, torch.float64)
    twin, _ = ec.encoder_step(init, c, enc_names, tokens, pos, d_enc, torch.float32, autocast=True)
    model = model.cuda()
    got, outs = hip_encoder(model, tokens, pos, d_enc)
    for i, (o, w) in enumerate(zip(outs, ref_out)):
        print("%s stage %d output rel-MSE %.2e" % (what, i, rel_mse(o.cpu(), w)))
        assert rel_mse(o.cpu(), w) < TOL_DECODE
    check_against_twin(got, ref, twin, what)
    got2, outs2 = hip_encoder(model, tokens, pos, d_enc)
    assert all(torch.equal(a, b) for a, b in zip(outs2, outs)) and all(torch.equal(got2[n], got[n]) for n in got)
