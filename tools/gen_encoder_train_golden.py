"""TEST INFRASTRUCTURE ONLY — writes tests/golden/encoder_train_tiny.npz: the reference's own `conv_in` (ActNorm), `encoder[i]` and
`top_down` under autograd with the stage-1 loss (trainer/Compressor_Trainer.py:43-52 without its EMD term), captured on the CPU.

Runs only where the upstream reference is present (imported through oracle/ref_import.py).  The Compressor of tests/golden/tiny_cfg.json
from its seed, lr 2e-3, warmup_iters 5, grad clip 1.0, B = 3, the cloud, the posterior draws and the kl_weight rule of
tools/gen_topdown_train_golden.py.  ActNorm does NOT stay at its init() state (shift = log_scale = 0, where its forward is the identity):
both are overwritten from a seeded generator (tests/encoder_train_checks.perturb_actnorm: shift 0.1 randn, log_scale 0.2 randn), in the
reference model and in the state the tests rebuild.  Stored:

    init_digest::*          digest of every tensor of the initial state_dict, ActNorm perturbed
    actnorm_shift, actnorm_log_scale   the perturbed ActNorm parameters (1, 8, 64)
    cloud, target           the seeded cloud (3, 64, 3) and the target clouds (the same cloud)
    tokens, pos             the grouped tokens (3, 8, 64) BEFORE ActNorm and the position condition (3, 32), from the oracle's pieces
                            (ldt_oracle.local_grouper, mini_pointnet) on the cloud: the leaves the frozen front hands to the encoder
    post_noise.i            the fixed posterior draws (3, 8, 40), in the order `Compressor.forward` takes them
    kl_weight, kl_norm, rec_norm   as the top-down fixture: a power of two that puts the KL part and the reconstruction part of the
                            reference gradient on decoder.*.prior.1.weight within a factor of 10
    enc_out.i, set, all_eps, loss, kl_loss, rec_loss   the reference's encoder stage outputs and top_down on them with the draws fixed
    d_enc_out.i, d_tokens, d_pos   the gradient of the loss at every stage output, at the tokens and at the position condition
    grad_digest::* / grad::*   the gradient of every encoder and top-down parameter (digest; an encoder parameter's tensor when it has
                            at most SMALL elements)
    encoder_names, topdown_names   the two parameter lists, in module order; every other parameter's gradient is None in the reference too
    traj_loss / traj_kl / traj_rec [10]   10 steps on the same batch: warm-up, loss, backward, clip_grad_norm_, torch.optim.Adam over the
                            encoder + top-down parameters
    oracle_grad_relmse      the worst rel-MSE of the float64 restatement from the oracle's pieces (tests/encoder_train_checks.chain_step:
                            act_norm, residual_block, final_layer, chained into topdown_train_checks.top_down) against the reference's
                            gradients — asserted <= 1e-10 here

    python tools/gen_encoder_train_golden.py
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
    model.eval(); model.init()
    init = copy.deepcopy(model.state_dict())
    import ldt_amd
    from ldt_amd.compressor_train import encoder_parameters, topdown_parameters
    torch.manual_seed(SEED)
    ours = ldt_amd.Compressor(c)
    ours.init()
    ours = ours.state_dict()
    assert ours.keys() == init.keys() and all(torch.equal(ours[k], init[k]) for k in init), "ldt_amd.Compressor's default init differs from upstream's"
    shift, log_scale = ec.perturb_actnorm(init)
    model.load_state_dict(init)
    assert torch.equal(model.conv_in.shift, shift) and torch.equal(model.conv_in.log_scale, log_scale) and bool(model.conv_in.initialized)
    enc_names = [n for n, _ in encoder_parameters(ldt_amd.Compressor(c))]
    top_names = [n for n, _ in topdown_parameters(ldt_amd.Compressor(c))]
    names = enc_names + top_names
    params = dict(model.named_parameters())
    assert not set(enc_names) & set(top_names) and [n for n in params if n in set(names)] == names
    g = torch.Generator().manual_seed(11)
    N, T, L, z = c.outsize, c.z_scales, c.n_layers, c.z_dim
    cloud = torch.randn(B, N, 3, generator=g)
    cloud = cloud - cloud.mean(1, keepdim=True)
    cloud = cloud / cloud.norm(dim=-1).amax(1)[:, None, None]
    post_noise = [torch.randn(B, T, z, generator=g) for _ in range(L)]
    with torch.no_grad():                                     # the frozen front, from the oracle's pieces (ldt_oracle.compressor_encode's lines)
        centers, tokens, _, _ = O.local_grouper(init, "group", cloud, O.linear(init, "input", cloud), T, N // T * 2)
        pos = O.mini_pointnet(init, "pos_embedding", centers)
        want = O.compressor_encode(init, c, cloud, post_noise)["enc_out"]
    tokens, pos = tokens.detach().clone(), pos.detach().clone()
    target = cloud

    draws = []
    Net.sample = lambda mu, logvar: mu + torch.exp(logvar / 2.) * draws.pop(0).to(mu)      # the draws fixed; channels-first like mu

    def ref_terms(tk, ps):
        """The reference's conv_in, encoder[i] (Network.py:200-205) and top_down on the leaves -> (set, kl_loss, all_eps, stage outputs)."""
        draws[:] = [t.transpose(1, 2) for t in post_noise]
        x = model.conv_in(tk.transpose(1, 2))
        outs = []
        for layer in model.encoder:
            x, o = layer(x, ps)
            outs.append(o)
        tdn = model.top_down(outs)
        assert not draws
        return tdn["set"], torch.cat(tdn["kls"], dim=1).mean(), torch.cat(tdn["all_eps"], dim=1).transpose(1, 2), outs

    # ---- kl_weight: the two parts of the gradient on the prior heads within a factor of 10 (the top-down fixture's rule)
    heads = [n for n in top_names if n.endswith(".prior.1.weight")]
    tk, ps = tokens.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    pts, kl_loss, all_eps, outs = ref_terms(tk, ps)
    for o, w in zip(outs, want):                              # the leaves ARE what the oracle's encode feeds its encoder
        assert rel_mse(o.detach().transpose(1, 2), w) < 1e-10
        o.retain_grad()
    rec_loss = cd_l1(pts, target)
    g_kl = torch.autograd.grad(kl_loss, [params[n] for n in heads], retain_graph=True)
    g_rec = torch.autograd.grad(rec_loss, [params[n] for n in heads], retain_graph=True)
    n_kl, n_rec = float(torch.cat([t.reshape(-1) for t in g_kl]).norm()), float(torch.cat([t.reshape(-1) for t in g_rec]).norm())
    kl_weight = float(2.0 ** round(np.log2(n_rec / n_kl)))                 # a power of two: exact in every format
    print("prior.1.weight gradient norms: KL (unit weight) %.4e, reconstruction %.4e -> kl_weight %g (KL part %.4e)" % (n_kl, n_rec, kl_weight, kl_weight * n_kl))
    assert 0.1 <= kl_weight * n_kl / n_rec <= 10
    loss = kl_weight * kl_loss + rec_loss
    loss.backward()
    grads = {n: params[n].grad.detach().clone() for n in names}
    assert all(p.grad is None for n, p in params.items() if n not in names), "a parameter outside the two lists got a gradient"
    out = {"cloud": cloud, "target": target, "encoder_names": np.array(enc_names), "topdown_names": np.array(top_names), "lr": cfg.opt.lr,
           "warmup_iters": cfg.opt.warmup_iters, "grad_norm_clip_value": cfg.opt.grad_norm_clip_value, "seed": SEED, "kl_weight": kl_weight,
           "kl_norm": kl_weight * n_kl, "rec_norm": n_rec, "tokens": tokens, "pos": pos, "actnorm_shift": shift.clone(),
           "actnorm_log_scale": log_scale.clone(), "d_tokens": tk.grad.detach().clone(), "d_pos": ps.grad.detach().clone(),
           "set": pts.detach().clone(), "all_eps": all_eps.detach().clone(), "loss": float(loss), "kl_loss": float(kl_loss), "rec_loss": float(rec_loss)}
    out.update({"init_digest::" + n: digest(v) for n, v in init.items()})
    out.update({"post_noise.%d" % i: t for i, t in enumerate(post_noise)})
    out.update({"enc_out.%d" % i: o.detach().transpose(1, 2).contiguous().clone() for i, o in enumerate(outs)})
    out.update({"d_enc_out.%d" % i: o.grad.detach().transpose(1, 2).contiguous().clone() for i, o in enumerate(outs)})
    out.update({"grad_digest::" + n: digest(v) for n, v in grads.items()})
    out.update({"grad::" + n: grads[n] for n in enc_names if grads[n].numel() <= SMALL})

    # ---- the float64 restatement from the oracle's pieces must reproduce them
    o_grads, o_loss, o_set, o_eps, o_enc = ec.chain_step(init, c, names, tokens, pos, post_noise, target, torch.float64, kl_weight)
    per = {n: rel_mse(o_grads[n], grads[n]) for n in names}
    per.update({k: rel_mse(o_grads[k], out[k]) for k in ["d_tokens", "d_pos"] + ["d_enc_out.%d" % i for i in range(L)]})
    worst = max(per.values())
    print("float64 restatement vs reference: worst gradient rel-MSE %.3e (%s), loss %.9f vs %.9f, kl %.9f vs %.9f, set rel-MSE %.3e, eps rel-MSE %.3e"
          % (worst, max(per, key=per.get), o_loss[0], float(loss), o_loss[1], float(kl_loss), rel_mse(o_set, pts), rel_mse(o_eps, all_eps)))
    assert worst <= 1e-10, "the restatement does not reproduce the reference's gradients"
    out["oracle_grad_relmse"] = worst

    # ---- 10 steps of the reference on the same batch
    model.zero_grad()
    plist = [params[n] for n in names]
    opt = torch.optim.Adam(plist, lr=cfg.opt.lr, betas=(cfg.opt.beta1, cfg.opt.beta2), weight_decay=cfg.opt.weight_decay)
    traj = []
    for i in range(ITERS):
        if i < cfg.opt.warmup_iters:
            for grp in opt.param_groups:
                grp["lr"] = cfg.opt.lr * min(float(i + 1) / max(cfg.opt.warmup_iters, 1), 1.0)
        opt.zero_grad()
        pts, kl_loss, _, _ = ref_terms(tokens, pos)
        rec_loss = cd_l1(pts, target)
        loss = kl_weight * kl_loss + rec_loss
        loss.backward()
        torch.nn.utils.clip_grad_norm_(plist, cfg.opt.grad_norm_clip_value)
        opt.step()
        traj.append((float(loss), float(kl_loss), float(rec_loss)))
    print("10 steps: loss %.6f -> %.6f (kl %.4f -> %.4f, rec %.4f -> %.4f)" % (traj[0][0], traj[-1][0], traj[0][1], traj[-1][1], traj[0][2], traj[-1][2]))
    assert traj[-1][0] < traj[0][0]
    t = torch.tensor(traj, dtype=torch.float64)
    out["traj_loss"], out["traj_kl"], out["traj_rec"] = t[:, 0].clone(), t[:, 1].clone(), t[:, 2].clone()
    save("encoder_train_tiny", **out)
    p = os.path.join(ROOT, "tests", "golden", "encoder_train_tiny.npz")
    print("%s: %d bytes" % (p, os.path.getsize(p)))
    assert os.path.getsize(p) <= 1 << 20


if __name__ == "__main__":
    main()
