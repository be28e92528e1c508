"""TEST INFRASTRUCTURE ONLY — writes tests/golden/decoder_train_tiny.npz: the reference's own Compressor decoder under autograd with the Chamfer
reconstruction loss, captured on the CPU.

Runs only where the upstream reference is present (imported through oracle/ref_import.py).  The Compressor of tests/golden/tiny_cfg.json
(hidden 64, 2 heads of 32, 3 levels, z = 40, 8 latent tokens, 64 set points) with lr 2e-3, warmup_iters 5, grad clip 1.0 (the opt block of
score_train_tiny.npz: at the tiny config's own lr 1e-4 / 2000 warm-up iterations ten steps move nothing), B = 3.  Stored:

    init_digest::*          digest of every tensor of the initial Compressor state_dict.  The weights themselves are `torch.manual_seed(33);
                            Compressor(cfg.compressor)` — ldt_amd.Compressor draws the same default init as upstream, asserted here tensor
                            by tensor — so the test rebuilds them from the seed.  digest(t) = float64 [sum, sum of squares, <t, cos(0.37 i)>]
    eps, target             the fixed latents (3, 8, 120) and the target clouds (3, 64, 3), from a seeded generator
    set, loss, d_eps        `model.sample((B, N), given_eps=eps)`, `CD_loss(set, target, 'l1')` restated over the reference's pure-torch
                            `chamfer_python.distChamfer` (evaluation/loss.py:71-78 calls the CUDA extension; same quantities), and the
                            gradient of the loss with respect to eps
    grad_digest::* / grad::*  the gradient of every decoder-side parameter: its digest, and the tensor itself when it has at most SMALL elements
    param_names             the decoder-side parameters, in module order; every other parameter's gradient is None in the reference too
                            (asserted here)
    traj_loss [10]          10 steps on the same batch: warm-up, loss, backward, clip_grad_norm_, torch.optim.Adam over the decoder-side
                            parameters (the reference's stage-1 optimizer, trainer/Compressor_Trainer.py, without its EMD / KL terms)
    oracle_grad_relmse      the worst rel-MSE, over the gradients and d_eps, of oracle.ldt_oracle.compressor_decode + autograd (float64, on
                            the float64 copy of the weights) against the reference's fp32 gradients — asserted <= 1e-10 here

    python tools/gen_decoder_train_golden.py
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import ldt_oracle as O  # noqa: E402
from oracle import ref_import as R  # noqa: E402
from oracle.gen_golden import save  # noqa: E402

ITERS, B, SEED = 10, 3, 33
SMALL = 4096          # tensors of at most this many elements are stored verbatim next to their digest


def rel_mse(a, b):
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).sum() / (b ** 2).sum().clamp_min(1e-300))


def digest(t):
    t = torch.as_tensor(t).detach().double().reshape(-1)
    return torch.stack([t.sum(), (t * t).sum(), (t * torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64))).sum()])


def train_cfg():
    with open(os.path.join(ROOT, "tests", "golden", "tiny_cfg.json")) as f:
        cfg = R.dict2ns(json.load(f))
    cfg.opt.lr, cfg.opt.warmup_iters, cfg.opt.grad_norm_clip_value = 2e-3, 5, 1.0
    return cfg


def is_decoder_side(name):
    p = name.split(".")
    return p[0] in ("output", "init_set") or (p[0] == "decoder" and (p[2] == "ln" or (p[2] == "att1" and p[3] in
                                                                     ("fc_q", "fc_kv", "fc_o", "norm1", "norm2", "mlp"))))


def main():
    R.setup()
    from evaluation.ChamferDistancePytorch.chamfer_python import distChamfer
    from model.Compressor.Network import Compressor

    def cd_l1(esti, shapes):                                  # evaluation/loss.py:71-78 over the pure-torch distances
        d1, d2, _, _ = distChamfer(esti, shapes)
        return torch.mean(torch.sqrt(d1)) + torch.mean(torch.sqrt(d2))

    cfg = train_cfg()
    c = cfg.compressor
    torch.manual_seed(SEED)
    model = Compressor(c)
    model.eval(); model.init()
    init = copy.deepcopy(model.state_dict())
    import ldt_amd
    torch.manual_seed(SEED)
    ours = ldt_amd.Compressor(c)
    ours.init()
    ours = ours.state_dict()
    assert ours.keys() == init.keys() and all(torch.equal(ours[k], init[k]) for k in init), "ldt_amd.Compressor's default init differs from upstream's"
    names = [n for n, _ in model.named_parameters() if is_decoder_side(n)]
    assert names == [n for n, _ in __import__("ldt_amd.compressor_train", fromlist=["x"]).decoder_parameters(ldt_amd.Compressor(c))]
    g = torch.Generator().manual_seed(7)
    N, T = c.outsize, c.z_scales
    eps = torch.randn(B, T, c.n_layers * c.z_dim, generator=g)
    target = torch.randn(B, N, 3, generator=g)
    target = target - target.mean(1, keepdim=True)
    target = target / target.norm(dim=-1).amax(1)[:, None, None]
    params = dict(model.named_parameters())
    out = {"eps": eps, "target": target, "param_names": np.array(names), "lr": cfg.opt.lr, "warmup_iters": cfg.opt.warmup_iters,
           "grad_norm_clip_value": cfg.opt.grad_norm_clip_value, "seed": SEED}
    out.update({"init_digest::" + n: digest(v) for n, v in init.items()})

    # ---- iteration 0: the reference's forward, loss and gradients
    e = eps.clone().requires_grad_(True)
    pts = model.sample((B, N), given_eps=e)
    loss = cd_l1(pts, target)
    loss.backward()
    grads = {n: params[n].grad.detach().clone() for n in names}
    assert all(p.grad is None for n, p in params.items() if n not in names), "a posterior-side parameter got a gradient"
    out["set"], out["loss"], out["d_eps"] = pts.detach().clone(), float(loss), e.grad.detach().clone()
    out.update({"grad_digest::" + n: digest(v) for n, v in grads.items()})
    out.update({"grad::" + n: v for n, v in grads.items() if v.numel() <= SMALL})

    # ---- the oracle in float64 must reproduce them
    sd = {k: v.detach().clone().double() for k, v in init.items()}
    leaves = [sd[n].requires_grad_(True) for n in names]
    e64 = eps.double().requires_grad_(True)
    o_pts = O.compressor_decode(sd, c, e64)
    o_loss = cd_l1(o_pts, target.double())
    o_loss.backward()
    per = {n: rel_mse(p.grad, grads[n]) for n, p in zip(names, leaves)}
    per["d_eps"] = rel_mse(e64.grad, out["d_eps"])
    worst = max(per.values())
    print("float64 oracle vs reference: worst gradient rel-MSE %.3e (%s), loss %.9f vs %.9f, set rel-MSE %.3e"
          % (worst, max(per, key=per.get), float(o_loss), float(loss), rel_mse(o_pts, pts)))
    assert worst <= 1e-10, "the oracle does not reproduce the reference's gradients"
    out["oracle_grad_relmse"] = worst

    # ---- 10 steps of the reference on the same batch
    model.zero_grad()
    plist = [params[n] for n in names]
    opt = torch.optim.Adam(plist, lr=cfg.opt.lr, betas=(cfg.opt.beta1, cfg.opt.beta2), weight_decay=cfg.opt.weight_decay)
    losses = []
    for i in range(ITERS):
        if i < cfg.opt.warmup_iters:
            for grp in opt.param_groups:
                grp["lr"] = cfg.opt.lr * min(float(i + 1) / max(cfg.opt.warmup_iters, 1), 1.0)
        opt.zero_grad()
        loss = cd_l1(model.sample((B, N), given_eps=eps), target)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(plist, cfg.opt.grad_norm_clip_value)
        opt.step()
        losses.append(float(loss))
    print("10 steps: loss %.6f -> %.6f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]
    out["traj_loss"] = torch.tensor(losses, dtype=torch.float64)
    save("decoder_train_tiny", **out)
    p = os.path.join(ROOT, "tests", "golden", "decoder_train_tiny.npz")
    print("%s: %d bytes" % (p, os.path.getsize(p)))
    assert os.path.getsize(p) <= 1 << 20


if __name__ == "__main__":
    main()
