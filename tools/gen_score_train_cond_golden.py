"""TEST INFRASTRUCTURE ONLY — writes tests/golden/score_train_cond.npz: the reference's own Score training step on a ViPC condition pair,
captured on the CPU.  Runs only where the upstream reference is present (imported through oracle/ref_import.py).

The step is the reference's completion `Trainer.update_score(eps, condition=(pts_condition, img_condition), cates=, discrete=True)`
(completion_trainer/Latent_SDE_Trainer.py:113-145).  The Scores are built with `condition: False`: such a Score accepts the embedded pair
(score.py:129-133) and needs no ConditionNet (and so no torchvision).  Both members of the pair are leaf tensors with requires_grad, so the
reference's `loss.backward()` also leaves the gradient with respect to them.  Models, options, latents and conditions:
tests/train_cond_checks.py (MODELS holds the layouts, so that the tests rebuild the very configs):

    x_*   2 heads x 64, 3 blocks (0 and 2 cross-attend), B 3, T 40, S 24: 20 iterations (idx [20, B], loss [20], twin_loss_dev)
    y_*   16 heads x 8, 2 blocks, B 4, T 32, S 32: one iteration
    z_*   4 heads x 32, 2 blocks, B 2, T 24, S 40, three classes AND a condition (the image condition is dropped, score.py:135): one iteration

Per model, as tools/gen_score_train_golden.py records them: init_digest::*, param_names, idx, loss, grad0_digest::* (iteration 0, before
clipping), grad0::* verbatim for the tensors of at most 1024 elements, cates (z), the digests of the latents and of the condition pair
(drawn again from their seeds by the tests), and
    dcond_pts (B, hidden, S), dcond_img (B, t_dim; absent for z)      the reference's gradient with respect to the pair, iteration 0, verbatim
    twin_grad_relmse::<name>, twin_grad_relmse_all, twin_dcond_relmse::pts / ::img, twin_loss_dev (x)
                                 the distances of a bf16 twin (oracle.ldt_oracle.score_forward under autocast, autograd, clip, Adam) from
                                 the reference: the yardsticks tests/test_gpu_train_cond.py holds the HIP path to.

The script asserts that the oracle in fp32 reproduces the reference's gradients — the condition's included — to <= 1e-10 rel-MSE.

    python tools/gen_score_train_cond_golden.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_score_train_golden as G  # noqa: E402
import train_cond_checks as tc  # noqa: E402
from oracle import ref_import as R  # noqa: E402
from oracle.gen_checkpoint_golden import torch2_optimizer_compat  # noqa: E402
from oracle.gen_golden import save, tiny_cfg  # noqa: E402


def run(key, out):
    import completion_trainer.Latent_SDE_Trainer as T
    from diffusion.diffusion_continuous import DiffusionVPSDE
    from model.Compressor.Network import Compressor
    from model.scorenet.score import Score
    m = tc.MODELS[key]
    iters = m["iters"]
    cfg = tc.set_train_options(tc.apply_overrides(tiny_cfg(N=50), key), key)
    torch.manual_seed(21)
    score, comp = Score(cfg.score), Compressor(cfg.compressor)
    comp.eval(); comp.init()
    init = copy.deepcopy(score.state_dict())
    import ldt_amd                                            # the tests rebuild the initial weights from the seed: same draws?
    torch.manual_seed(21)
    ours = ldt_amd.Score(cfg.score).state_dict()
    assert ours.keys() == init.keys() and all(torch.equal(ours[k], init[k]) for k in init), "ldt_amd.Score's default init differs from upstream's"
    names = [n for n, _ in score.named_parameters()]
    with R.quiet():
        tr = T.Trainer(cfg, score, comp, "cpu")
    torch2_optimizer_compat(tr.optimizer)
    eps, (pts0, img0) = tc.latents(key), tc.conditions(key)
    cates = tc.cates_of(key)
    pts, img = pts0.clone().requires_grad_(True), img0.clone().requires_grad_(True)
    grads, dcond = {}, {}
    orig_clip = T.clip_grad_norm_

    def spy_clip(params, max_norm, *a, **k):
        params = list(params)
        if not grads:
            grads.update({n: p.grad.detach().clone() for n, p in zip(names, params)})
            dcond["pts"] = pts.grad.detach().clone()
            dcond["img"] = None if img.grad is None else img.grad.detach().clone()
        return orig_clip(params, max_norm, *a, **k)

    T.clip_grad_norm_ = spy_clip
    idxs, losses = [], []
    try:
        for i in range(iters):
            idx, _ = G.draw(i, eps.shape, cfg.sde.train_N)
            tr.itr = i
            torch.manual_seed(1000 + i)
            loss = tr.update_score(eps, condition=(pts, img), cates=cates, discrete=True)
            idxs.append(idx); losses.append(float(loss))
            pts.grad = None; img.grad = None
    finally:
        T.clip_grad_norm_ = orig_clip
    if cates is not None:                                     # score.py:135: the label displaces the image condition
        assert dcond["img"] is None or float(dcond["img"].abs().max()) == 0.0
        dcond["img"] = None
    tag = key + "_"
    out.update({tag + "init_digest::" + n: G.digest(v) for n, v in init.items()})
    out.update({tag + "grad0_digest::" + n: G.digest(v) for n, v in grads.items()})
    out.update({tag + "grad0::" + n: v for n, v in grads.items() if v.numel() <= G.SMALL})
    out[tag + "param_names"] = np.array(names)
    out[tag + "idx"], out[tag + "loss"] = torch.stack(idxs), torch.tensor(losses, dtype=torch.float64)
    out[tag + "eps_digest"], out[tag + "pts_digest"], out[tag + "img_digest"] = G.digest(eps), G.digest(pts0), G.digest(img0)
    out[tag + "dcond_pts"] = dcond["pts"]
    if dcond["img"] is not None:
        out[tag + "dcond_img"] = dcond["img"]
    if cates is not None:
        out[tag + "cates"] = cates

    # the oracle in fp32 (must reproduce the reference's gradients) and the bf16 twin (the yardsticks)
    sde = DiffusionVPSDE(cfg.sde)
    for twin in (False, True):
        sd = {k: v.clone() for k, v in init.items()}
        leaves = [sd[n].requires_grad_(True) for n in names]
        opt = torch.optim.Adam(leaves, lr=cfg.opt.lr, betas=(cfg.opt.beta1, cfg.opt.beta2), weight_decay=cfg.opt.weight_decay)
        dev = 0.0
        for i in range(iters if twin else 1):
            idx, eta = G.draw(i, eps.shape, cfg.sde.train_N)
            for grp in opt.param_groups:
                grp["lr"] = cfg.opt.lr * min(float(i + 1) / max(cfg.opt.warmup_iters, 1), 1.0) if i < cfg.opt.warmup_iters else grp["lr"]
            opt.zero_grad()
            p, im = pts0.clone().requires_grad_(True), img0.clone().requires_grad_(True)
            t = torch.linspace(1.0, cfg.sde.sample_time_eps, cfg.sde.train_N).index_select(0, idx)
            with torch.autocast("cpu", torch.bfloat16, enabled=twin):
                loss = tc.oracle_loss(sd, cfg, eps, t, sde.e2int_f(t), sde.var(t), eta, p, im, cates=cates)
            loss.float().backward()
            if i == 0:
                per = {n: G.rel_mse(q.grad, grads[n]) for n, q in zip(names, leaves)}
                allg = G.rel_mse(torch.cat([q.grad.reshape(-1) for q in leaves]), torch.cat([grads[n].reshape(-1) for n in names]))
                pc = {"pts": G.rel_mse(p.grad, dcond["pts"])}
                if dcond["img"] is not None:
                    pc["img"] = G.rel_mse(im.grad, dcond["img"])
                if not twin:
                    worst = max(max(per.values()), allg, max(pc.values()))
                    print("%sfp32 oracle vs reference: worst gradient rel-MSE %.3e (condition: %s), loss %.9f vs %.9f"
                          % (tag, worst, ", ".join("%s %.1e" % kv for kv in pc.items()), float(loss), losses[0]))
                    assert worst <= 1e-10, "the oracle does not reproduce the reference's gradients"
                else:
                    out.update({tag + "twin_grad_relmse::" + n: v for n, v in per.items()})
                    out.update({tag + "twin_dcond_relmse::" + n: v for n, v in pc.items()})
                    out[tag + "twin_grad_relmse_all"] = allg
                    print("%stwin gradient rel-MSE: all %.3e, per tensor %.3e .. %.3e; condition %s"
                          % (tag, allg, min(per.values()), max(per.values()), ", ".join("%s %.3e" % kv for kv in pc.items())))
            dev = max(dev, abs(float(loss) - losses[i]) / losses[i])
            torch.nn.utils.clip_grad_norm_(leaves, cfg.opt.grad_norm_clip_value)
            opt.step()
        if twin and iters > 1:
            out[tag + "twin_loss_dev"] = dev
            print("%stwin_loss_dev over %d iterations: %.3e (losses %.4f -> %.4f)" % (tag, iters, dev, losses[0], losses[-1]))


def main():
    R.setup()
    out = {}
    for key in tc.MODELS:
        run(key, out)
    big = [k for k, v in out.items() if torch.is_tensor(v) and v.numel() > G.SMALL and "_dcond_" not in k]
    assert not big, big
    save("score_train_cond", **out)


if __name__ == "__main__":
    main()
