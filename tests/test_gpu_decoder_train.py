"""GPU (-m gpu): one training step of the Compressor's decoder on the HIP path (ldt_amd/compressor_train.py: DecoderTrainStep;
CompressorTrainer.update_decoder; ldt_amd.losses.cd_loss), whole.

Case `tiny`, against tests/golden/decoder_train_tiny.npz (tools/gen_decoder_train_golden.py: the reference's own Compressor under autograd
with CD_loss restated over its pure-torch Chamfer; hidden 64, 2 heads of 32, 3 levels, 8 latent tokens, 64 set points, B = 3):
  * the loss within 1e-3 relative (DESIGN.md section 4.11's bar), the decoded set at the decode bar of the golden tests (rel-MSE 1e-4)
  * every gradient and d_eps: rel-MSE <= 2 x max(the bf16 twin's on that tensor, the twin's on all of them) — the project's yardstick
    (section 4.11).  The twin is oracle.ldt_oracle.compressor_decode under torch.autocast("cpu", bfloat16) + autograd, computed here; the
    reference gradients are the float64 oracle's (the capture asserts they equal the reference's to 1e-10), tied to the fixture through
    the captured tensors and digests.  All three backward passes — the HIP step's, the reference's and the twin's — start from ONE
    gradient with respect to the set, the reference's own d loss / d set: the Chamfer loss is not continuous in the set (a perturbation
    of the set of the size bf16 leaves, rel-MSE 1e-5, flips 1 to 5 of the 384 nearest-neighbour assignments), and started from each
    run's OWN loss gradient the figures measure which assignments flipped, not the backward: with float64 arithmetic throughout and
    nothing but such a perturbation of the set, the rel-MSE of decoder.2.att1.fc_q.bias ranges over 8e-4 .. 6e-3 from draw to draw (the
    twin's own draw: 1.6e-3, the HIP step's: 5.1e-3; norm1.bias of the same block 1.7e-3 and 6.5e-3).  The same reason for which
    decoder_train_checks teacher-forces the Chamfer gradient on the kernel's indices.  What the shared start leaves out is asserted
    too: the step's own d loss / d set per element against float64 on its own (validated) indices; the step END TO END from its own
    loss gradient, every tensor within 2 x the twin's — in the ragged case exactly as the yardstick is stated (each run from its own
    start, against the reference), in the tiny case, where the flips decide that figure, with each side's own validated assignments
    forced into the float64 reference's loss (check_end_to_end_on_own_indices: the step against the reference on the step's indices,
    the twin against the reference on the twin's), so that a backward that is wrong only from the step's own start still shows; and
    the 10-step trajectory
  * 10 update_decoder steps on the same batch: the loss trajectory's worst relative deviation from the reference's <= 2 x the twin's; the loss
    falls; every posterior-side parameter is bit-unchanged with .grad None; Compressor.sample afterwards decodes with the NEW weights
Case `ragged`, against the float64 oracle + autograd with the same yardstick: hidden 128, 4 heads, 2 levels, z 20, 24 latent tokens, 300 of
320 prior rows under a keep mask, B 2 — the shipped width at the smallest set with a partial chunk of queries and a partial 16-row tile:
  * exact: dprior of a row no sample kept is exactly 0
A second forward + backward repeats bit for bit.

Before the step existed every test here ended at the missing `ldt_amd.compressor_train`."""
import copy
import os

import numpy as np
import pytest
import torch

import decoder_train_checks as dc
from conftest import GOLDEN, rel_mse

pytestmark = pytest.mark.gpu
_CACHE = {}
TOL_DECODE = 1e-4                                                       # tests/test_gpu_path.py


def golden():
    if "g" not in _CACHE:
        z = np.load(os.path.join(GOLDEN, "decoder_train_tiny.npz"))
        _CACHE["g"] = {k: (torch.from_numpy(np.asarray(z[k])) if z[k].dtype.kind in "fiu" else z[k]) for k in z.files}
    return _CACHE["g"]


def digest(t):
    t = torch.as_tensor(t).detach().double().cpu().reshape(-1)
    return torch.stack([t.sum(), (t * t).sum(), (t * torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64))).sum()])


def same_digest(got, want, numel):
    return float((got - want).abs().max()) <= 1e-9 * (float(want[1]) * numel) ** 0.5 + 1e-300


def train_cfg(tiny_cfg):
    g = golden()
    cfg = copy.deepcopy(tiny_cfg)
    cfg.opt.lr, cfg.opt.warmup_iters, cfg.opt.grad_norm_clip_value = float(g["lr"]), int(g["warmup_iters"]), float(g["grad_norm_clip_value"])
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


def oracle_step(init, ccfg, names, eps, target, dtype, keep_mask=None, autocast=False, d_set=None):
    """compressor_decode + CD_loss('l1') + autograd on a copy of the weights -> ({name: grad, 'd_eps': grad, 'd_set': d loss / d set}, loss,
    set, leaves).  d_set: the gradient with respect to the set to start the backward from, in place of this run's own (see the module text)."""
    from oracle import ldt_oracle as O
    sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in init.items()}
    leaves = [sd[n].requires_grad_(True) for n in names]
    e = eps.detach().clone().to(dtype).requires_grad_(True)
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        pts = O.compressor_decode(sd, ccfg, e, keep_mask=keep_mask)
    pts.retain_grad()
    loss = dc.cd_loss_torch(pts.to(dtype), target.to(dtype), "l1")
    if d_set is None:
        loss.backward()
    else:
        pts.backward(d_set.to(pts.dtype))
    grads = {n: p.grad for n, p in zip(names, leaves)}
    grads["d_eps"] = e.grad
    grads["d_set"] = pts.grad
    return grads, float(loss.detach()), pts.detach(), (sd, leaves)


def check_against_twin(got, ref, twin, what, twin_ref=None):
    """got / ref / twin: {name: tensor}.  Per tensor and concatenated: rel-MSE(got) <= 2 x max(twin's on it, twin's overall).
    twin_ref: the reference the twin is measured against, when it is not `ref` (each side against the reference on its OWN indices)."""
    names = [n for n in ref if n != "d_set"]
    twin_ref = ref if twin_ref is None else twin_ref
    cat = lambda d: torch.cat([d[n].detach().double().cpu().reshape(-1) for n in names])
    t_all = rel_mse(cat(twin), cat(twin_ref))
    worst, over = 0.0, []
    for n in names:                                                     # every figure is printed before anything is asserted
        e, t = rel_mse(got[n].cpu(), ref[n]), rel_mse(twin[n], twin_ref[n])
        bar = 2 * max(t, t_all)
        worst = max(worst, e / bar)
        print("%s %-40s rel-MSE %.3e  twin %.3e  bar %.3e  ratio %.2f" % (what, n, e, t, bar, e / bar))
        if not e <= bar:
            over.append("%s: %.3e > %.3e" % (n, e, bar))
    assert not over, "%s: gradient rel-MSE above 2 x the bf16 twin's: %s" % (what, "; ".join(over))
    e_all = rel_mse(cat(got), cat(ref))
    print("%s: gradient rel-MSE, all tensors: %.3e = %.2f x the twin's %.3e; worst per-tensor ratio to its bar %.2f" % (what, e_all, e_all / t_all, t_all, worst))
    assert e_all <= 2 * t_all


def hip_step(model, eps, target, keep_mask=None, num_points=None, d_set=None):
    """forward, cd_loss with its gradient, backward from `d_set` (the step's own loss gradient when None)
    -> ({name: grad, 'd_eps', 'd_set': the step's own loss gradient}, loss, set)."""
    from ldt_amd import losses
    from ldt_amd.compressor_train import DecoderTrainStep, decoder_parameters
    step = DecoderTrainStep(model)
    pts = step.forward(eps.cuda(), num_points=num_points, keep_mask=keep_mask)
    loss, own = losses.cd_loss(pts, target.cuda(), "l1", want_grad=True)
    d_eps = step.backward(own if d_set is None else d_set.float().cuda())
    got = {n: p.grad.detach().clone() for n, p in decoder_parameters(model)}
    got["d_eps"] = d_eps.clone()
    got["d_set"] = own
    return got, float(loss), pts


def forced_reference(init, ccfg, names, eps, target, idx1, idx2, keep_mask=None):
    """The float64 reference with GIVEN nearest-neighbour assignments forced into its loss: its own decoded set, the Chamfer gradient of
    decoder_train_checks.cd_grad on (idx1 [B, n] into the target, idx2 [B, m] into the set), its own backward -> {name: grad, 'd_eps'}.
    With the reference's own indices this is the reference's gradient itself (checked where it is used)."""
    from oracle import ldt_oracle as O
    sd = {k: (v.detach().clone().double() if v.is_floating_point() else v.clone()) for k, v in init.items()}
    with torch.no_grad():
        ref_set = O.compressor_decode(sd, ccfg, eps.double(), keep_mask=keep_mask)
    d_set, _ = dc.cd_grad(ref_set, target, idx1, idx2, "l1")
    return oracle_step(init, ccfg, names, eps, target, torch.float64, keep_mask=keep_mask, d_set=d_set)[0]


def check_end_to_end_on_own_indices(own, pts, free, free_set, init, ccfg, names, eps, target, ref, ref_set, what):
    """The step end to end (its own loss gradient) against the float64 reference with the STEP's own, validated nearest-neighbour
    assignments forced into the reference's loss; the bar: 2 x the bf16 twin's distance from the reference with the TWIN's own
    assignments forced.  What a flipped assignment does to the gradient is thereby in neither figure; everything else — the set's
    error through the direction vectors and weights of the loss gradient, and the whole backward from the step's own start — is."""
    from ldt_amd import ops
    _, i1, _, i2 = ops.chamfer_nn(pts, target.cuda())
    dc.assert_valid_argmin(pts.cpu(), target, i1, what + " idx1")
    dc.assert_valid_argmin(target, pts.cpu(), i2, what + " idx2")
    _, _, r1, r2 = dc.dist_chamfer_torch(ref_set, target.double())
    same = forced_reference(init, ccfg, names, eps, target, r1, r2)      # the helper on the reference's own indices IS the reference
    assert all(rel_mse(same[n], ref[n]) <= 1e-20 for n in same if n != "d_set")
    _, _, t1, t2 = dc.dist_chamfer_torch(free_set.double(), target.double())
    flips = lambda a, b: int((a.cpu().long() != b).sum())
    print("%s: nearest-neighbour assignments that differ from the reference's: the step's %d + %d, the twin's %d + %d of %d + %d"
          % (what, flips(i1, r1), flips(i2, r2), flips(t1, r1), flips(t2, r2), r1.numel(), r2.numel()))
    check_against_twin(own, forced_reference(init, ccfg, names, eps, target, i1, i2), free, what,
                       twin_ref=forced_reference(init, ccfg, names, eps, target, t1, t2))


def check_own_loss_gradient(pts, target, d_set, what):
    """The step's own d loss / d set, per element, against float64 teacher-forced on the kernel's indices, each first checked to be a valid
    argmin (decoder_train_checks: the bound of test_gpu_cd_loss.py, here on the decoded set itself)."""
    import kernel_checks as kc
    from ldt_amd import ops
    _, i1, _, i2 = ops.chamfer_nn(pts, target.cuda())
    dc.assert_valid_argmin(pts.cpu(), target, i1, what + " idx1")
    dc.assert_valid_argmin(target, pts.cpu(), i2, what + " idx2")
    ref, tol = dc.cd_grad(pts.cpu(), target, i1, i2, "l1")
    r = kc.assert_elementwise(d_set.cpu(), ref, tol, what + " d_set")
    print("%s: the step's own d loss / d set against float64 on its own indices: max err/tol %.3f" % (what, r))


def test_tiny_gradients_loss_and_set_against_the_fixture(tiny_cfg):
    from ldt_amd.compressor_train import decoder_parameters
    g = golden()
    cfg = train_cfg(tiny_cfg)
    model, init = tiny_model(cfg)
    names = [n for n, _ in decoder_parameters(model)]
    assert names == [str(n) for n in g["param_names"]]
    eps, target = g["eps"], g["target"]
    ref, ref_loss, ref_set, _ = oracle_step(init, cfg.compressor, names, eps, target, torch.float64)
    assert abs(ref_loss - float(g["loss"])) <= 1e-6 * float(g["loss"]) and rel_mse(ref_set, g["set"]) < 1e-10
    assert rel_mse(ref["d_eps"], g["d_eps"]) <= 1e-9
    for n in names:                                                     # the float64 oracle IS the captured reference, tensor by tensor
        d, w = digest(ref[n]), g["grad_digest::" + n]                    # (float64 against the captured fp32 gradient: rel-MSE ~1e-12)
        assert abs(float(d[1] - w[1])) <= 1e-5 * float(w[1]) and abs(float(d[2] - w[2])) <= 1e-5 * (float(w[1]) * ref[n].numel()) ** 0.5, n
        if "grad::" + n in g:
            assert rel_mse(ref[n], g["grad::" + n]) <= 1e-9, n
    twin, _, _, _ = oracle_step(init, cfg.compressor, names, eps, target, torch.float32, autocast=True, d_set=ref["d_set"])
    model = model.cuda()
    got, loss, pts = hip_step(model, eps, target, d_set=ref["d_set"])
    print("tiny: loss %.6f vs the reference's %.6f (rel %.2e); set rel-MSE %.2e" % (loss, float(g["loss"]), abs(loss - float(g["loss"])) / float(g["loss"]),
                                                                                 rel_mse(pts.cpu(), g["set"])))
    assert abs(loss - float(g["loss"])) <= 1e-3 * float(g["loss"])
    assert tuple(pts.shape) == tuple(g["set"].shape) and rel_mse(pts.cpu(), g["set"]) < TOL_DECODE
    check_against_twin(got, ref, twin, "tiny")
    check_own_loss_gradient(pts, target, got["d_set"], "tiny")
    named = dict(model.named_parameters())
    assert all(p.grad is None for n, p in named.items() if n not in names)
    got2, loss2, pts2 = hip_step(model, eps, target, d_set=ref["d_set"])   # fixed order everywhere: the same bits
    assert loss2 == loss and torch.equal(pts2, pts) and all(torch.equal(got2[n], got[n]) for n in got)
    # end to end on the step's own loss gradient
    own, _, _ = hip_step(model, eps, target)
    free, _, free_set, _ = oracle_step(init, cfg.compressor, names, eps, target, torch.float32, autocast=True)
    for n in ("decoder.2.att1.fc_q.bias", "decoder.2.att1.norm1.norm.bias", "d_eps"):     # against the untouched reference: the flips' figure
        print("tiny, own loss gradient, reference untouched: %-34s rel-MSE %.3e (the twin on ITS own: %.3e)" % (n, rel_mse(own[n].cpu(), ref[n]), rel_mse(free[n], ref[n])))
    check_end_to_end_on_own_indices(own, pts, free, free_set, init, cfg.compressor, names, eps, target, ref, ref_set, "tiny, own loss gradient")


def test_tiny_ten_steps_of_update_decoder(tiny_cfg):
    import ldt_amd
    from ldt_amd.compressor_train import decoder_parameters
    from oracle import ldt_oracle as O
    g = golden()
    cfg = train_cfg(tiny_cfg)
    model, init = tiny_model(cfg)
    names = [n for n, _ in decoder_parameters(model)]
    eps, target = g["eps"], g["target"]
    ref = g["traj_loss"].tolist()
    # the bf16 twin's trajectory: autocast + autograd + clip + Adam on the same batch
    _, _, _, (sd, leaves) = oracle_step(init, cfg.compressor, names, eps, target, torch.float32, autocast=True)
    opt = torch.optim.Adam(leaves, lr=cfg.opt.lr, betas=(cfg.opt.beta1, cfg.opt.beta2), weight_decay=cfg.opt.weight_decay)
    twin_dev = 0.0
    for i in range(len(ref)):
        if i < cfg.opt.warmup_iters:
            for grp in opt.param_groups:
                grp["lr"] = cfg.opt.lr * min(float(i + 1) / max(cfg.opt.warmup_iters, 1), 1.0)
        opt.zero_grad()
        with torch.autocast("cpu", torch.bfloat16):
            pts = O.compressor_decode(sd, cfg.compressor, eps)
        loss = dc.cd_loss_torch(pts.float(), target, "l1")
        loss.backward()
        torch.nn.utils.clip_grad_norm_(leaves, cfg.opt.grad_norm_clip_value)
        opt.step()
        twin_dev = max(twin_dev, abs(float(loss) - ref[i]) / ref[i])
    tr = ldt_amd.CompressorTrainer(cfg, model, "cuda")
    assert tr.optimizer is None                                          # nothing allocated before the first call
    frozen = {n: p.detach().clone() for n, p in model.named_parameters() if n not in names}
    losses = []
    for i in range(len(ref)):
        loss, rec = tr.update_decoder({"tr_points": target}, eps=eps.cuda())
        assert loss.dim() == 0 and loss.is_cuda and torch.equal(loss, rec)
        losses.append(float(loss))
    dev = max(abs(a - b) / b for a, b in zip(losses, ref))
    print("tiny 10-step trajectory: %.4f -> %.4f (reference %.4f -> %.4f); worst relative deviation %.3e = %.2f x the twin's %.3e"
          % (losses[0], losses[-1], ref[0], ref[-1], dev, dev / twin_dev, twin_dev))
    assert dev <= 2 * twin_dev
    assert losses[-1] < losses[0]
    assert tr.itr == len(ref) and isinstance(tr.optimizer, ldt_amd.AdamEMA) and not tr.optimizer.apply_ema
    assert tuple(tr.last_eps_grad.shape) == tuple(eps.shape)
    named = dict(model.named_parameters())
    for n, v in frozen.items():
        assert torch.equal(named[n].detach(), v) and named[n].grad is None, n
    assert all(not torch.equal(named[n].detach().cpu(), init[n]) for n in names if named[n].numel() > 1)
    # sample() decodes with the weights the optimizer wrote through raw pointers
    now = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    want = O.compressor_decode(now, cfg.compressor, eps)
    pts = model.sample((eps.shape[0], target.shape[1]), given_eps=eps.cuda()).cpu()
    assert rel_mse(pts, want) < TOL_DECODE and rel_mse(pts, g["set"]) > 100 * TOL_DECODE
    # without `eps` the step encodes the batch itself, under no_grad and in evaluation mode, and hands the caller's mode back
    model.train()
    loss, _ = tr.update_decoder({"tr_points": target})
    assert model.training and bool(loss.isfinite()) and tr.itr == len(ref) + 1
    assert tuple(tr.last_eps_grad.shape) == tuple(eps.shape) and bool(tr.last_eps_grad.isfinite().all())
    for n, v in frozen.items():
        assert torch.equal(dict(model.named_parameters())[n].detach(), v), n


def test_ragged_step_under_a_keep_mask(tiny_cfg):
    import ldt_amd
    from ldt_amd.compressor_train import decoder_parameters
    c = copy.deepcopy(tiny_cfg.compressor)
    c.hidden_dim, c.num_heads, c.n_layers, c.z_dim, c.z_scales, c.max_outputs, c.outsize = 128, 4, 2, 20, 24, 320, 300
    B, N = 2, 300
    torch.manual_seed(5)
    model = ldt_amd.Compressor(c)
    model.init()
    with torch.no_grad():                                               # away from the default init's gamma = 1, beta = 0
        for n, p in model.named_parameters():
            if ".norm1." in n or ".norm2." in n:
                p.add_(0.2 * torch.randn(p.shape))
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    names = [n for n, _ in decoder_parameters(model)]
    g = torch.Generator().manual_seed(9)
    eps = torch.randn(B, c.z_scales, c.n_layers * c.z_dim, generator=g)
    target = torch.randn(B, 200, 3, generator=g) * 0.5                  # a target of another length than the set
    keep = torch.stack([torch.randperm(c.max_outputs, generator=g) < N for _ in range(B)])
    keep[:, 17] = False                                                 # a row no sample keeps (each sample then keeps one row fewer: put one back)
    for b in range(B):
        spare = torch.nonzero(~keep[b]).flatten()
        spare = spare[spare != 17]
        keep[b, spare[:N - int(keep[b].sum())]] = True
    assert bool((keep.sum(1) == N).all()) and not bool(keep[:, 17].any())
    ref, ref_loss, ref_set, _ = oracle_step(init, c, names, eps, target, torch.float64, keep_mask=keep)
    twin, _, _, _ = oracle_step(init, c, names, eps, target, torch.float32, keep_mask=keep, autocast=True, d_set=ref["d_set"])
    model = model.cuda()
    got, loss, pts = hip_step(model, eps, target, keep_mask=keep, num_points=N, d_set=ref["d_set"])
    print("ragged: loss %.6f vs float64 %.6f (rel %.2e); set rel-MSE %.2e" % (loss, ref_loss, abs(loss - ref_loss) / ref_loss, rel_mse(pts.cpu(), ref_set)))
    assert abs(loss - ref_loss) <= 1e-3 * ref_loss and rel_mse(pts.cpu(), ref_set) < TOL_DECODE
    check_against_twin(got, ref, twin, "ragged")
    check_own_loss_gradient(pts, target, got["d_set"], "ragged")
    held = keep.sum(0)
    assert bool((got["init_set.prior"].cpu()[held == 0] == 0).all()) and int((held == 0).sum()) >= 1
    assert bool((ref["init_set.prior"][held == 0] == 0).all())
    got2, loss2, _ = hip_step(model, eps, target, keep_mask=keep, num_points=N, d_set=ref["d_set"])
    assert loss2 == loss and all(torch.equal(got2[n], got[n]) for n in got)
    # end to end on the step's own loss gradient, as the yardstick is stated: every run from its own start, against the reference
    own, _, _ = hip_step(model, eps, target, keep_mask=keep, num_points=N)
    free = oracle_step(init, c, names, eps, target, torch.float32, keep_mask=keep, autocast=True)[0]
    check_against_twin(own, ref, free, "ragged, own loss gradient")
