"""GPU (-m gpu): one training step of the Compressor's top-down half on the HIP path (ldt_amd/compressor_train.py: TopDownTrainStep;
CompressorTrainer.update_topdown; Compressor.bottom_up), whole.  The yardstick is the one of test_gpu_decoder_train.py (DESIGN.md sections
4.11 / 4.15): per tensor, rel-MSE <= 2 x max(the bf16 twin's on that tensor, the twin's overall), the twin being the float64 restatement
(tests/topdown_train_checks.top_down, from the oracle's pieces) under torch.autocast("cpu", bfloat16).

Case `tiny`, against tests/golden/topdown_train_tiny.npz (tools/gen_topdown_train_golden.py: the reference's own Compressor.top_down under
autograd with kl_weight * cat(kls).mean() + CD_loss; hidden 64, 2 heads of 32, 3 levels, 8 latent tokens, 64 set points, B = 3):
  * the set at the decode bar (rel-MSE 1e-4), the loss and kl_loss within 1e-3 relative
  * the step's forward on the inference path's own encoder outputs (Compressor.bottom_up) against Compressor.forward(post_noise=...): set
    and all_eps at the decode bar; DecoderTrainStep on the step's all_eps gives the step's set bit for bit (the shared pieces are shared)
  * every gradient and every d_enc_out[i] within the yardstick in four variants: (1) from ONE d_set, the reference's (section 4.15's
    reason: Chamfer assignment flips); (2) d_set = 0, the KL path alone; (3) kl_scale = 0, the reconstruction path through the posterior
    alone; (4) end to end from the step's own loss gradient with each side's own validated assignments forced into the float64
    reference's loss
  * 10 update_topdown steps on one batch: the loss falls, its worst relative deviation from the reference trajectory <= 2 x the twin's,
    every bottom-up parameter bit-unchanged with .grad None, Compressor.forward afterwards runs on the NEW weights
Case `ragged`, against the float64 restatement: hidden 128, 4 heads, 2 levels, z 20, 24 tokens, B 2, 600 of 640 prior rows under a keep
mask: level 1's wide attention is 24 queries on 600 keys (three chunks, the last partial, and a partial 16-row tile), level 0 the self
form; each run from its own start; the gradient of a prior row no sample kept is exactly 0.
A second forward + backward repeats bit for bit, d_enc_out included.

Before the step existed every test here ended at the missing `TopDownTrainStep`, `update_topdown` or `bottom_up`."""
import copy
import os

import numpy as np
import pytest
import torch

import decoder_train_checks as dc
import topdown_train_checks as tc
from conftest import GOLDEN, rel_mse
from test_gpu_decoder_train import check_against_twin, check_own_loss_gradient, digest, same_digest

pytestmark = pytest.mark.gpu
_CACHE = {}
TOL_DECODE = 1e-4                                                       # tests/test_gpu_path.py


def golden():
    if "g" not in _CACHE:
        z = np.load(os.path.join(GOLDEN, "topdown_train_tiny.npz"))
        _CACHE["g"] = {k: (torch.from_numpy(np.asarray(z[k])) if z[k].dtype.kind in "fiu" else z[k]) for k in z.files}
    return _CACHE["g"]


def train_cfg(tiny_cfg):
    g = golden()
    cfg = copy.deepcopy(tiny_cfg)
    cfg.opt.lr, cfg.opt.warmup_iters, cfg.opt.grad_norm_clip_value = float(g["lr"]), int(g["warmup_iters"]), float(g["grad_norm_clip_value"])
    cfg.opt.kl_weight = float(g["kl_weight"])
    return cfg


def tiny_model(cfg):
    """The fixture's initial Compressor (rebuilt from its seed, checked against the digests) -> (model on the CPU, its state_dict copy)."""
    import ldt_amd
    g = golden()
    torch.manual_seed(int(g["seed"]))
    model = ldt_amd.Compressor(cfg.compressor)
    model.init()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for k, v in init.items():
        assert same_digest(digest(v), g["init_digest::" + k], v.numel()), "initial weights differ from the fixture's: " + k
    return model, init


def fixture_inputs(L):
    g = golden()
    return [g["enc_out.%d" % i] for i in range(L)], [g["post_noise.%d" % i] for i in range(L)], g["target"]


def hip_step(model, enc_out, post_noise, target, kl_scale, keep_mask=None, num_points=None, d_set=None, rec=True):
    """forward, cd_loss with its gradient, backward from `d_set` (the step's own loss gradient when None; zeros when not rec)
    -> ({name: grad, 'd_enc_out.i', 'd_set': the step's own loss gradient}, (kl_sample_sum, rec_loss), set, all_eps)."""
    from ldt_amd import losses
    from ldt_amd.compressor_train import TopDownTrainStep, topdown_parameters
    step = TopDownTrainStep(model)
    pts, all_eps, kls = step.forward([t.cuda() for t in enc_out], [t.cuda() for t in post_noise], num_points=num_points, keep_mask=keep_mask)
    loss, own = losses.cd_loss(pts, target.cuda(), "l1", want_grad=True)
    start = torch.zeros_like(own) if not rec else (own if d_set is None else d_set.float().cuda())
    d_enc = step.backward(start, kl_scale)
    assert d_enc is step.d_enc_out and len(d_enc) == len(enc_out)
    got = {n: p.grad.detach().clone() for n, p in topdown_parameters(model)}
    got.update({"d_enc_out.%d" % i: t.clone() for i, t in enumerate(d_enc)})
    got["d_set"] = own
    return got, (kls, float(loss)), pts, all_eps


def n_kl_of(c, B):
    return c.n_layers * B * c.z_dim * c.z_scales


def test_tiny_gradients_loss_and_set_against_the_fixture(tiny_cfg):
    from ldt_amd.compressor_train import DecoderTrainStep, topdown_parameters
    g = golden()
    cfg = train_cfg(tiny_cfg)
    c, kw = cfg.compressor, float(g["kl_weight"])
    model, init = tiny_model(cfg)
    names = [n for n, _ in topdown_parameters(model)]
    assert names == [str(n) for n in g["param_names"]]
    enc_out, post_noise, target = fixture_inputs(c.n_layers)
    B = target.shape[0]
    ks = kw / n_kl_of(c, B)
    print("tiny: kl_weight %g; on decoder.*.prior.1.weight the reference gradient's KL part has norm %.4e, its reconstruction part %.4e"
          % (kw, float(g["kl_norm"]), float(g["rec_norm"])))
    assert 0.1 <= float(g["kl_norm"]) / float(g["rec_norm"]) <= 10
    ref, ref_loss, ref_set, ref_eps, _ = tc.oracle_step(init, c, names, enc_out, post_noise, target, torch.float64, kw)
    assert abs(ref_loss[0] - float(g["loss"])) <= 1e-6 * float(g["loss"]) and rel_mse(ref_set, g["set"]) < 1e-10 and rel_mse(ref_eps, g["all_eps"]) < 1e-10
    for i in range(c.n_layers):
        assert rel_mse(ref["d_enc_out.%d" % i], g["d_enc_out.%d" % i]) <= 1e-9
    for n in names:                                                     # the float64 restatement IS the captured reference, tensor by tensor
        d, w = digest(ref[n]), g["grad_digest::" + n]
        assert abs(float(d[1] - w[1])) <= 1e-5 * float(w[1]) and abs(float(d[2] - w[2])) <= 1e-5 * (float(w[1]) * ref[n].numel()) ** 0.5, n
        if "grad::" + n in g:
            assert rel_mse(ref[n], g["grad::" + n]) <= 1e-9, n
    model = model.cuda()
    # (1) from ONE d_set, the reference's
    twin = tc.oracle_step(init, c, names, enc_out, post_noise, target, torch.float32, kw, autocast=True, d_set=ref["d_set"])[0]
    got, (kls, rec_loss), pts, all_eps = hip_step(model, enc_out, post_noise, target, ks, d_set=ref["d_set"])
    kl_loss = float(kls.sum()) / n_kl_of(c, B)
    loss = kw * kl_loss + rec_loss
    print("tiny: loss %.6f vs the reference's %.6f (rel %.2e); kl_loss %.6f vs %.6f (rel %.2e); set rel-MSE %.2e; all_eps rel-MSE %.2e"
          % (loss, float(g["loss"]), abs(loss - float(g["loss"])) / float(g["loss"]), kl_loss, float(g["kl_loss"]),
             abs(kl_loss - float(g["kl_loss"])) / abs(float(g["kl_loss"])), rel_mse(pts.cpu(), g["set"]), rel_mse(all_eps.cpu(), g["all_eps"])))
    assert tuple(kls.shape) == (B, c.n_layers)
    assert tuple(pts.shape) == tuple(g["set"].shape) and rel_mse(pts.cpu(), g["set"]) < TOL_DECODE
    assert abs(loss - float(g["loss"])) <= 1e-3 * float(g["loss"])
    assert abs(kl_loss - float(g["kl_loss"])) <= 1e-3 * abs(float(g["kl_loss"]))
    check_against_twin(got, ref, twin, "tiny (1) one d_set")
    check_own_loss_gradient(pts, target, got["d_set"], "tiny")
    named = dict(model.named_parameters())
    assert all(p.grad is None for n, p in named.items() if n not in names)
    got2, _, pts2, eps2 = hip_step(model, enc_out, post_noise, target, ks, d_set=ref["d_set"])   # fixed order everywhere: the same bits
    assert torch.equal(pts2, pts) and torch.equal(eps2, all_eps) and all(torch.equal(got2[n], got[n]) for n in got)
    # the shared pieces are shared: the decoder step on the step's latents decodes the same bits
    assert torch.equal(DecoderTrainStep(model).forward(all_eps), pts)
    # (2) d_set = 0: the KL path alone
    ref_kl = tc.oracle_step(init, c, names, enc_out, post_noise, target, torch.float64, kw, rec=False)[0]
    twin_kl = tc.oracle_step(init, c, names, enc_out, post_noise, target, torch.float32, kw, autocast=True, rec=False)[0]
    got_kl = hip_step(model, enc_out, post_noise, target, ks, rec=False)[0]
    assert bool((got_kl["output.weight"] == 0).all()) and bool((ref_kl["output.weight"] == 0).all())
    check_against_twin(got_kl, ref_kl, twin_kl, "tiny (2) KL alone")
    # (3) kl_scale = 0: the reconstruction path through the posterior alone
    ref_rec = tc.oracle_step(init, c, names, enc_out, post_noise, target, torch.float64, 0.0, d_set=ref["d_set"])[0]
    twin_rec = tc.oracle_step(init, c, names, enc_out, post_noise, target, torch.float32, 0.0, autocast=True, d_set=ref["d_set"])[0]
    got_rec = hip_step(model, enc_out, post_noise, target, 0.0, d_set=ref["d_set"])[0]
    check_against_twin(got_rec, ref_rec, twin_rec, "tiny (3) reconstruction alone")
    # (4) end to end from the step's own loss gradient, each side's own validated assignments forced into the float64 reference's loss
    from ldt_amd import ops
    own = hip_step(model, enc_out, post_noise, target, ks)[0]
    free, _, free_set, _, _ = tc.oracle_step(init, c, names, enc_out, post_noise, target, torch.float32, kw, autocast=True)

    def forced(idx1, idx2):
        d_set, _ = dc.cd_grad(ref_set, target, idx1, idx2, "l1")
        return tc.oracle_step(init, c, names, enc_out, post_noise, target, torch.float64, kw, d_set=d_set)[0]

    _, i1, _, i2 = ops.chamfer_nn(pts, target.cuda())
    dc.assert_valid_argmin(pts.cpu(), target, i1, "tiny idx1"); dc.assert_valid_argmin(target, pts.cpu(), i2, "tiny idx2")
    _, _, r1, r2 = dc.dist_chamfer_torch(ref_set, target.double())
    same = forced(r1, r2)                                               # the helper on the reference's own indices IS the reference
    assert all(rel_mse(same[n], ref[n]) <= 1e-20 for n in same if n != "d_set")
    _, _, t1, t2 = dc.dist_chamfer_torch(free_set.double(), target.double())
    check_against_twin(own, forced(i1, i2), free, "tiny (4) own loss gradient", twin_ref=forced(t1, t2))


def test_tiny_forward_against_the_inference_path(tiny_cfg):
    """The step's unfused forward on Compressor.bottom_up's outputs against Compressor.forward, which runs the same bottom-up code and the
    fused top-down kernels; bottom_up itself against the fixture's encoder outputs (the float64 oracle's)."""
    from ldt_amd.compressor_train import TopDownTrainStep
    g = golden()
    cfg = train_cfg(tiny_cfg)
    c = cfg.compressor
    model, _ = tiny_model(cfg)
    model = model.cuda().eval()
    enc_ref, post_noise, _ = fixture_inputs(c.n_layers)
    cloud = g["cloud"].cuda()
    bup = model.bottom_up(cloud)
    assert sorted(bup) == ["centers", "fps_idx", "knn_idx", "max", "outputs"] and len(bup["outputs"]) == c.n_layers
    B, T = cloud.shape[0], c.z_scales
    for o, want in zip(bup["outputs"], enc_ref):
        assert tuple(o.shape) == (B, c.hidden_dim, T) and o.transpose(1, 2).is_contiguous()     # channels-first views of token-major buffers
        assert rel_mse(o.transpose(1, 2).cpu(), want) < TOL_DECODE
    fwd = model(cloud, post_noise=[t.cuda() for t in post_noise], want_kl=True)
    assert torch.equal(fwd["fps_idx"], bup["fps_idx"]) and torch.equal(fwd["centers"], bup["centers"]) and torch.equal(fwd["max"], bup["max"])
    pts, all_eps, kls = TopDownTrainStep(model).forward([o.transpose(1, 2) for o in bup["outputs"]], [t.cuda() for t in post_noise])
    print("tiny forward vs the inference path: set rel-MSE %.2e, all_eps rel-MSE %.2e, kl_sample_sum rel-MSE %.2e"
          % (rel_mse(pts, fwd["set"]), rel_mse(all_eps, fwd["all_eps"]), rel_mse(kls, fwd["kl_sample_sum"])))
    assert rel_mse(pts, fwd["set"]) < TOL_DECODE and rel_mse(all_eps, fwd["all_eps"]) < TOL_DECODE
    again = model.bottom_up(cloud)["outputs"]
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(again, bup["outputs"]))     # fresh buffers, the same bits


def test_tiny_ten_steps_of_update_topdown(tiny_cfg):
    import ldt_amd
    from ldt_amd.compressor_train import topdown_parameters
    from oracle import ldt_oracle as O
    g = golden()
    cfg = train_cfg(tiny_cfg)
    c, kw = cfg.compressor, float(g["kl_weight"])
    model, init = tiny_model(cfg)
    names = [n for n, _ in topdown_parameters(model)]
    enc_out, post_noise, target = fixture_inputs(c.n_layers)
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
            pts, _, kls = tc.top_down(sd, c, enc_out, post_noise)
        loss = kw * torch.cat([k.float() for k in kls], dim=1).mean() + dc.cd_loss_torch(pts.float(), target, "l1")
        loss.backward()
        torch.nn.utils.clip_grad_norm_(leaves, cfg.opt.grad_norm_clip_value)
        opt.step()
        twin_dev = max(twin_dev, abs(float(loss) - ref[i]) / abs(ref[i]))
    tr = ldt_amd.CompressorTrainer(cfg, model, "cuda")
    assert tr.topdown_optimizer is None and tr.optimizer is None         # nothing allocated before the first call
    frozen = {n: p.detach().clone() for n, p in model.named_parameters() if n not in names}
    enc_d, nz_d = [t.cuda() for t in enc_out], [t.cuda() for t in post_noise]
    losses = []
    for i in range(len(ref)):
        loss, kl_loss, rec_loss = tr.update_topdown({"tr_points": target}, enc_out=enc_d, post_noise=nz_d)
        assert loss.dim() == 0 and loss.is_cuda and kl_loss.dim() == 0 and rec_loss.dim() == 0
        assert abs(float(loss) - (kw * float(kl_loss) + float(rec_loss))) <= 1e-6 * abs(float(loss)) + 1e-7
        losses.append(float(loss))
    dev = max(abs(a - b) / abs(b) for a, b in zip(losses, ref))
    print("tiny 10-step trajectory: %.4f -> %.4f (reference %.4f -> %.4f); worst relative deviation %.3e = %.2f x the twin's %.3e"
          % (losses[0], losses[-1], ref[0], ref[-1], dev, dev / twin_dev, twin_dev))
    assert dev <= 2 * twin_dev
    assert losses[-1] < losses[0]
    assert tr.itr == len(ref) and isinstance(tr.topdown_optimizer, ldt_amd.AdamEMA) and not tr.topdown_optimizer.apply_ema and tr.optimizer is None
    assert len(tr.last_enc_out_grad) == c.n_layers and all(tuple(t.shape) == tuple(e.shape) for t, e in zip(tr.last_enc_out_grad, enc_out))
    named = dict(model.named_parameters())
    for n, v in frozen.items():
        assert torch.equal(named[n].detach(), v) and named[n].grad is None, n
    assert all(not torch.equal(named[n].detach().cpu(), init[n]) for n in names if named[n].numel() > 1)
    # Compressor.forward runs on the weights the optimizer wrote through raw pointers
    now = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    want = O.compressor_encode(now, c, g["cloud"], post_noise)
    model.eval()
    fwd = model(g["cloud"].cuda(), post_noise=nz_d)
    assert rel_mse(fwd["set"].cpu(), want["set"]) < TOL_DECODE and rel_mse(fwd["set"].cpu(), g["set"]) > 100 * TOL_DECODE
    assert rel_mse(fwd["all_eps"].cpu(), want["all_eps"]) < TOL_DECODE
    # without `enc_out` / `post_noise` the step runs bottom_up itself, under no_grad and in evaluation mode, and hands the caller's mode back
    model.train()
    loss, kl_loss, rec_loss = tr.update_topdown({"tr_points": g["cloud"]})
    assert model.training and bool(loss.isfinite()) and tr.itr == len(ref) + 1
    assert all(bool(t.isfinite().all()) for t in tr.last_enc_out_grad)
    for n, v in frozen.items():
        assert torch.equal(dict(model.named_parameters())[n].detach(), v), n


def test_ragged_step_under_a_keep_mask(tiny_cfg):
    import ldt_amd
    from ldt_amd.compressor_train import topdown_parameters
    c = copy.deepcopy(tiny_cfg.compressor)
    c.hidden_dim, c.num_heads, c.n_layers, c.z_dim, c.z_scales, c.max_outputs, c.outsize = 128, 4, 2, 20, 24, 640, 600
    B, N, kw = 2, 600, float(golden()["kl_weight"])
    torch.manual_seed(5)
    model = ldt_amd.Compressor(c)
    model.init()
    with torch.no_grad():                                               # away from the default init's gamma = 1, beta = 0
        for n, p in model.named_parameters():
            if ".norm1." in n or ".norm2." in n:
                p.add_(0.2 * torch.randn(p.shape))
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    names = [n for n, _ in topdown_parameters(model)]
    g = torch.Generator().manual_seed(9)
    enc_out = [torch.randn(B, c.z_scales, c.hidden_dim, generator=g) for _ in range(c.n_layers)]
    post_noise = [torch.randn(B, c.z_scales, c.z_dim, generator=g) for _ in range(c.n_layers)]
    target = torch.randn(B, 200, 3, generator=g) * 0.5                  # a target of another length than the set
    keep = torch.stack([torch.randperm(c.max_outputs, generator=g) < N for _ in range(B)])
    keep[:, 17] = False                                                 # a row no sample keeps (each sample then keeps one row fewer: put one back)
    for b in range(B):
        spare = torch.nonzero(~keep[b]).flatten()
        spare = spare[spare != 17]
        keep[b, spare[:N - int(keep[b].sum())]] = True
    assert bool((keep.sum(1) == N).all()) and not bool(keep[:, 17].any())
    ks = kw / n_kl_of(c, B)
    ref, ref_loss, ref_set, ref_eps, _ = tc.oracle_step(init, c, names, enc_out, post_noise, target, torch.float64, kw, keep_mask=keep)
    free = tc.oracle_step(init, c, names, enc_out, post_noise, target, torch.float32, kw, keep_mask=keep, autocast=True)[0]
    model = model.cuda()
    own, (kls, rec_loss), pts, all_eps = hip_step(model, enc_out, post_noise, target, ks, keep_mask=keep, num_points=N)
    kl_loss = float(kls.sum()) / n_kl_of(c, B)
    loss = kw * kl_loss + rec_loss
    print("ragged: loss %.6f vs float64 %.6f (rel %.2e); kl_loss %.6f vs %.6f; set rel-MSE %.2e; all_eps rel-MSE %.2e"
          % (loss, ref_loss[0], abs(loss - ref_loss[0]) / abs(ref_loss[0]), kl_loss, ref_loss[1], rel_mse(pts.cpu(), ref_set), rel_mse(all_eps.cpu(), ref_eps)))
    assert abs(loss - ref_loss[0]) <= 1e-3 * abs(ref_loss[0]) and rel_mse(pts.cpu(), ref_set) < TOL_DECODE and rel_mse(all_eps.cpu(), ref_eps) < TOL_DECODE
    check_against_twin(own, ref, free, "ragged, own loss gradient")   # as the yardstick is stated: every run from its own start
    check_own_loss_gradient(pts, target, own["d_set"], "ragged")
    held = keep.sum(0)
    assert bool((own["init_set.prior"].cpu()[held == 0] == 0).all()) and int((held == 0).sum()) >= 1
    assert bool((ref["init_set.prior"][held == 0] == 0).all())
    own2, _, pts2, eps2 = hip_step(model, enc_out, post_noise, target, ks, keep_mask=keep, num_points=N)
    assert torch.equal(pts2, pts) and torch.equal(eps2, all_eps) and all(torch.equal(own2[n], own[n]) for n in own)
