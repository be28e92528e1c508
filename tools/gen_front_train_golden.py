"""TEST INFRASTRUCTURE ONLY — writes tests/golden/front_train_tiny.npz: the reference's own `input`, `group`, `pos_embedding`, `conv_in`,
`encoder[i]` and `top_down` in TRAINING mode under autograd with the stage-1 loss (trainer/Compressor_Trainer.py:43-52 without its EMD
term), captured on the CPU.

Runs only where the upstream reference is present (imported through oracle/ref_import.py, which also provides FPS).  The cloud, the
posterior draws, the perturbed ActNorm, the optimizer settings and the kl_weight rule are tools/gen_encoder_train_golden.py's.  The reference
runs in float64 (`model.double()`): the front holds discrete selections (three ReLUs and the max over the neighbours in the grouper, two
ReLUs and the max over the tokens in MiniPointnet), and a float64 restatement can reproduce fp32 gradients to 1e-10 only where no selection
flips between the two precisions.  Stored:

    init_digest::*          digest of every tensor of the initial state_dict (ActNorm perturbed, the BatchNorm buffers included)
    cloud, target, post_noise.i, kl_weight, lr, warmup_iters, grad_norm_clip_value, seed
    fps_idx, knn_idx        the grouping the reference ran at (oracle.ldt_oracle.fps / knn: an unordered neighbour set per centre)
    tokens, pos             the grouped tokens (3, 8, 64) BEFORE ActNorm and the position condition (3, 32) of the training-mode front
    sel::*                  the reference's selections (tests/front_train_checks.FRONT_SELECTIONS), rows in the order of knn_idx
    set, loss, kl_loss, rec_loss, d_tokens, d_pos
    grad_digest::* / grad::*   the gradient of every parameter (digest; a front parameter's tensor when it has at most SMALL elements)
    front_names             front_parameters, in module order
    bn::*                   the four BatchNorms' running_mean / running_var / num_batches_tracked after ONE training step
    traj_loss / traj_kl / traj_rec [10]   10 steps on the same batch: warm-up, loss, backward, clip_grad_norm_, torch.optim.Adam over ALL parameters
    oracle_grad_relmse      the worst rel-MSE of the float64 restatement (tests/front_train_checks.whole_step) against the reference's
                            gradients, the analytically zero ones (FRONT_DEAD) held against their live neighbours — asserted <= 1e-10 here
    twin_shares::*          the share of cells on which the bf16 twin of THIS fixture selects differently from float64 (asserted inside the
                            caps the GPU test holds the device to: 2 % of arg-max cells, 1 % of ReLU cells per layer)

    python tools/gen_front_train_golden.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ldt_oracle as O  # noqa: E402
from oracle import ref_import as R  # noqa: E402
from oracle.gen_golden import save  # noqa: E402
from tools.gen_decoder_train_golden import B, ITERS, SEED, SMALL, digest, rel_mse, train_cfg  # noqa: E402
import encoder_train_checks as ec  # noqa: E402
import front_train_checks as fc  # noqa: E402


def main():
    R.setup()
    from evaluation.ChamferDistancePytorch.chamfer_python import distChamfer
    import model.Compressor.Network as Net

    def cd_l1(esti, shapes):                                  # evaluation/loss.py:71-78 over the pure-torch distances
        d1, d2, _, _ = distChamfer(esti, shapes)
        return torch.mean(torch.sqrt(d1)) + torch.mean(torch.sqrt(d2))

    cfg = train_cfg()
    c = cfg.compressor
    torch.manual_seed(SEED)
    model = Net.Compressor(c)
    model.init()
    init = copy.deepcopy(model.state_dict())
    import ldt_amd
    from ldt_amd.compressor_train import encoder_parameters, front_parameters, topdown_parameters
    torch.manual_seed(SEED)
    ours = ldt_amd.Compressor(c)
    ours.init()
    assert ours.state_dict().keys() == init.keys() and all(torch.equal(ours.state_dict()[k], init[k]) for k in init)
    ec.perturb_actnorm(init)
    model.load_state_dict(init)
    model = model.double()
    model.train()                                             # the reference's trainer calls model.train() before the step
    fr_names = [n for n, _ in front_parameters(ours)]
    names = fr_names + [n for n, _ in encoder_parameters(ours)] + [n for n, _ in topdown_parameters(ours)]
    params = dict(model.named_parameters())
    assert sorted(names) == sorted(params)
    g = torch.Generator().manual_seed(11)
    N, T, L, z = c.outsize, c.z_scales, c.n_layers, c.z_dim
    cloud = torch.randn(B, N, 3, generator=g)
    cloud = cloud - cloud.mean(1, keepdim=True)
    cloud = cloud / cloud.norm(dim=-1).amax(1)[:, None, None]
    post_noise = [torch.randn(B, T, z, generator=g) for _ in range(L)]
    target = cloud
    fps_idx = O.fps(cloud, T)
    knn_idx = O.knn(N // T * 2, cloud, O.gather(cloud, fps_idx))

    draws = []
    Net.sample = lambda mu, logvar: mu + torch.exp(logvar / 2.) * draws.pop(0).to(mu)      # the draws fixed; channels-first like mu

    def ref_terms():
        """The reference's bottom_up and top_down on the cloud -> (set, kl_loss)."""
        draws[:] = [t.transpose(1, 2) for t in post_noise]
        tdn = model.top_down(model.bottom_up(cloud.double())["outputs"])
        assert not draws
        return tdn["set"], torch.cat(tdn["kls"], dim=1).mean()

    kl_weight = float(np.load(os.path.join(ROOT, "tests", "golden", "encoder_train_tiny.npz"))["kl_weight"])
    pts, kl_loss = ref_terms()
    rec_loss = cd_l1(pts, target.double())
    loss = kl_weight * kl_loss + rec_loss
    loss.backward()
    grads = {n: params[n].grad.detach().clone() for n in names}
    after = {k: v.detach().clone() for k, v in model.state_dict().items() if ("running_" in k or "num_batches" in k)}

    # ---- the float64 restatement must reproduce them, with its own selections
    o_grads, o_loss, tokens, pos, sel, bns = fc.whole_step(init, c, names, cloud, fps_idx, knn_idx, post_noise, target, torch.float64, kl_weight)
    per = {n: rel_mse(o_grads[n], grads[n]) for n in names if n not in fc.FRONT_DEAD}
    worst = max(per.values())
    for n, live in fc.FRONT_DEAD.items():                     # analytically zero: noise on both sides
        assert float(grads[n].abs().max()) <= 1e-12 * float(grads[live].abs().max()) and float(o_grads[n].abs().max()) <= 1e-12 * float(grads[live].abs().max()), n
    print("float64 restatement vs reference: worst gradient rel-MSE %.3e (%s), loss %.12f vs %.12f" % (worst, max(per, key=per.get), o_loss[0], float(loss.detach())))
    # (the loss to 1e-6 as the encoder fixture holds it: the oracle's pieces carry a few fp32 constants)
    assert worst <= 1e-10 and abs(o_loss[0] - float(loss.detach())) <= 1e-6 * abs(float(loss.detach())), "the restatement does not reproduce the reference"
    want = fc.running_after(init, bns)
    for k, v in after.items():
        assert float((want[k].double() - v.double()).abs().max()) <= 1e-12, k

    # ---- the bf16 twin of THIS fixture stays inside the selection caps
    _, _, _, _, tsel, _ = fc.whole_step(init, c, names, cloud, fps_idx, knn_idx, post_noise, target, torch.float32, kl_weight, twin=True)
    shares = fc.selection_shares(sel, tsel)
    print("bf16 twin selection shares: " + "  ".join("%s %.4f" % kv for kv in shares.items()))
    assert max(shares["arg"], shares["parg"]) <= 0.02 and max(shares[k] for k in ("mask1", "mask2", "mask3", "pmask1", "pmask2")) <= 0.01, "change the seed, not the caps"

    out = {"cloud": cloud, "target": target, "front_names": np.array(fr_names), "lr": cfg.opt.lr, "warmup_iters": cfg.opt.warmup_iters,
           "grad_norm_clip_value": cfg.opt.grad_norm_clip_value, "seed": SEED, "kl_weight": kl_weight, "fps_idx": fps_idx.int(), "knn_idx": knn_idx.int(),
           "tokens": tokens.float(), "pos": pos.float(), "d_tokens": o_grads["d_tokens"].float(), "d_pos": o_grads["d_pos"].float(),
           "set": pts.detach().float(), "loss": float(loss.detach()), "kl_loss": float(kl_loss.detach()), "rec_loss": float(rec_loss.detach()),
           "oracle_grad_relmse": worst}
    out.update({"init_digest::" + n: digest(v) for n, v in init.items()})
    out.update({"post_noise.%d" % i: t for i, t in enumerate(post_noise)})
    out.update({"sel::" + k: (v.to(torch.uint8) if v.dtype == torch.bool else v.int()) for k, v in sel.items()})
    out.update({"grad_digest::" + n: digest(v) for n, v in grads.items()})
    out.update({"grad::" + n: grads[n].float() for n in fr_names if grads[n].numel() <= SMALL})
    out.update({"bn::" + k: (v.float() if v.is_floating_point() else v) for k, v in after.items()})
    out.update({"twin_shares::" + k: v for k, v in shares.items()})

    # ---- 10 steps of the reference on the same batch, every parameter trained
    model.zero_grad()
    plist = [params[n] for n in names]
    opt = torch.optim.Adam(plist, lr=cfg.opt.lr, betas=(cfg.opt.beta1, cfg.opt.beta2), weight_decay=cfg.opt.weight_decay)
    traj = []
    for i in range(ITERS):
        if i < cfg.opt.warmup_iters:
            for grp in opt.param_groups:
                grp["lr"] = cfg.opt.lr * min(float(i + 1) / max(cfg.opt.warmup_iters, 1), 1.0)
        opt.zero_grad()
        pts, kl_loss = ref_terms()
        rec_loss = cd_l1(pts, target.double())
        loss = kl_weight * kl_loss + rec_loss
        loss.backward()
        torch.nn.utils.clip_grad_norm_(plist, cfg.opt.grad_norm_clip_value)
        opt.step()
        traj.append((float(loss.detach()), float(kl_loss.detach()), float(rec_loss.detach())))
    print("10 steps: loss %.6f -> %.6f (kl %.4f -> %.4f, rec %.4f -> %.4f)" % (traj[0][0], traj[-1][0], traj[0][1], traj[-1][1], traj[0][2], traj[-1][2]))
    assert traj[-1][0] < traj[0][0]
    t = torch.tensor(traj, dtype=torch.float64)
    out["traj_loss"], out["traj_kl"], out["traj_rec"] = t[:, 0].clone(), t[:, 1].clone(), t[:, 2].clone()
    save("front_train_tiny", **out)
    p = os.path.join(ROOT, "tests", "golden", "front_train_tiny.npz")
    print("%s: %d bytes" % (p, os.path.getsize(p)))
    assert os.path.getsize(p) <= 1 << 20


if __name__ == "__main__":
    main()
