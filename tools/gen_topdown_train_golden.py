"""TEST INFRASTRUCTURE ONLY — writes tests/golden/topdown_train_tiny.npz: the reference's own `Compressor.top_down` under autograd with the
stage-1 loss (trainer/Compressor_Trainer.py:43-52 without its EMD term), captured on the CPU.

Runs only where the upstream reference is present (imported through oracle/ref_import.py).  The Compressor of tests/golden/tiny_cfg.json
(hidden 64, 2 heads of 32, 3 levels, z = 40, 8 latent tokens, 64 set points) from its seed, lr 2e-3, warmup_iters 5, grad clip 1.0, B = 3, as
tools/gen_decoder_train_golden.py.  Stored:

    init_digest::*          digest of every tensor of the initial state_dict (`torch.manual_seed(33); Compressor(cfg.compressor)`:
                            ldt_amd.Compressor draws the same default init, asserted here tensor by tensor)
    cloud, target           the seeded cloud (3, 64, 3) the encoder outputs come from, and the target clouds (the same cloud)
    enc_out.i, post_noise.i the encoder outputs (3, 8, 64) of oracle.ldt_oracle.compressor_encode on the cloud, and the fixed posterior draws
                            (3, 8, 40), in the order `Compressor.forward` takes them
    kl_weight, kl_norm, rec_norm   the fixture's kl_weight — NOT the shipped 1e-6, whose gradient no test would see: chosen here so that on
                            decoder.*.prior.1.weight the KL part and the reconstruction part of the reference gradient have norms within a
                            factor of 10 — and the two norms
    set, all_eps, loss, kl_loss, rec_loss   the reference's `top_down(encoder_out)` with the draws fixed, `kl_weight * cat(kls).mean() +
                            CD_loss(set, target, 'l1')` restated over the reference's pure-torch Chamfer
    grad_digest::* / grad::* / d_enc_out.i   the gradient of every top-down parameter (digest; the tensor when it has at most SMALL elements)
                            and of every encoder output
    param_names             the top-down parameters, in module order; every other parameter's gradient is None in the reference too
    traj_loss / traj_kl / traj_rec [10]   10 steps on the same batch: warm-up, loss, backward, clip_grad_norm_, torch.optim.Adam over the
                            top-down parameters
    oracle_grad_relmse      the worst rel-MSE of the float64 restatement from the oracle's pieces (tests/topdown_train_checks.top_down:
                            residual_block, linear, decoder_block, initial_set) against the reference's gradients — asserted <= 1e-10 here

    python tools/gen_topdown_train_golden.py
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
import topdown_train_checks as tc  # noqa: E402


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
    from ldt_amd.compressor_train import topdown_parameters
    torch.manual_seed(SEED)
    ours = ldt_amd.Compressor(c)
    ours.init()
    ours = ours.state_dict()
    assert ours.keys() == init.keys() and all(torch.equal(ours[k], init[k]) for k in init), "ldt_amd.Compressor's default init differs from upstream's"
    names = [n for n, _ in topdown_parameters(ldt_amd.Compressor(c))]
    params = dict(model.named_parameters())
    assert [n for n in params if n in set(names)] == names
    g = torch.Generator().manual_seed(11)
    N, T, L, z = c.outsize, c.z_scales, c.n_layers, c.z_dim
    cloud = torch.randn(B, N, 3, generator=g)
    cloud = cloud - cloud.mean(1, keepdim=True)
    cloud = cloud / cloud.norm(dim=-1).amax(1)[:, None, None]
    post_noise = [torch.randn(B, T, z, generator=g) for _ in range(L)]
    with torch.no_grad():
        enc_out = [t.detach().clone() for t in O.compressor_encode(init, c, cloud, post_noise)["enc_out"]]
    target = cloud

    draws = []
    Net.sample = lambda mu, logvar: mu + torch.exp(logvar / 2.) * draws.pop(0).to(mu)      # the draws fixed; channels-first like mu

    def ref_terms(xs):
        draws[:] = [t.transpose(1, 2) for t in post_noise]
        tdn = model.top_down([x.transpose(1, 2) for x in xs])
        assert not draws
        return tdn["set"], torch.cat(tdn["kls"], dim=1).mean(), torch.cat(tdn["all_eps"], dim=1).transpose(1, 2)

    # ---- kl_weight: the two parts of the gradient on the prior heads within a factor of 10
    heads = [n for n in names if n.endswith(".prior.1.weight")]
    xs = [t.clone().requires_grad_(True) for t in enc_out]
    pts, kl_loss, all_eps = ref_terms(xs)
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
    assert all(p.grad is None for n, p in params.items() if n not in names), "a bottom-up parameter got a gradient"
    out = {"cloud": cloud, "target": target, "param_names": np.array(names), "lr": cfg.opt.lr, "warmup_iters": cfg.opt.warmup_iters,
           "grad_norm_clip_value": cfg.opt.grad_norm_clip_value, "seed": SEED, "kl_weight": kl_weight, "kl_norm": kl_weight * n_kl, "rec_norm": n_rec,
           "set": pts.detach().clone(), "all_eps": all_eps.detach().clone(), "loss": float(loss), "kl_loss": float(kl_loss), "rec_loss": float(rec_loss)}
    out.update({"init_digest::" + n: digest(v) for n, v in init.items()})
    out.update({"enc_out.%d" % i: t for i, t in enumerate(enc_out)})
    out.update({"post_noise.%d" % i: t for i, t in enumerate(post_noise)})
    out.update({"d_enc_out.%d" % i: x.grad.detach().clone() for i, x in enumerate(xs)})
    out.update({"grad_digest::" + n: digest(v) for n, v in grads.items()})
    out.update({"grad::" + n: v for n, v in grads.items() if v.numel() <= SMALL})

    # ---- the float64 restatement from the oracle's pieces must reproduce them
    o_grads, o_loss, o_set, o_eps, _ = tc.oracle_step(init, c, names, enc_out, post_noise, target, torch.float64, kl_weight)
    per = {n: rel_mse(o_grads[n], grads[n]) for n in names}
    per.update({"d_enc_out.%d" % i: rel_mse(o_grads["d_enc_out.%d" % i], out["d_enc_out.%d" % i]) for i in range(L)})
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
        pts, kl_loss, _ = ref_terms(enc_out)
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
    save("topdown_train_tiny", **out)
    p = os.path.join(ROOT, "tests", "golden", "topdown_train_tiny.npz")
    print("%s: %d bytes" % (p, os.path.getsize(p)))
    assert os.path.getsize(p) <= 1 << 20


if __name__ == "__main__":
    main()
