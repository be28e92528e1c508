"""TEST INFRASTRUCTURE ONLY — writes tests/golden/score_train_tiny.npz: the reference's own Score training step, captured on the CPU.

Runs only where the upstream reference is present (imported through oracle/ref_import.py).  The tiny config of tests/golden/tiny_cfg.json
(Score hidden 128, 2 heads of 64, 2 blocks, 8 tokens, z = 120) with lr 2e-3, warmup_iters 5, ema_decay 0.98, grad clip 1.0, B = 8 fixed
latents.  Stored:

    init_digest::*               digest of every tensor of the initial Score state_dict.  The weights themselves are `torch.manual_seed(21);
                                 Score(cfg.score)` — ldt_amd.Score draws the same default init as upstream, asserted here tensor by tensor —
                                 so the test rebuilds them from the seed and checks the digests.  (A committed file may hold 1 MiB; one
                                 copy of this Score is 2.2 MB.  digest(t) = float64 [sum, sum of squares, <t, cos(0.37 i)>].)
    eps                          the fixed latents (8, 8, 120)
    idx [20, 8], loss [20]       20 iterations of the reference's `Trainer.update_score(eps, discrete=True)` with `tr.itr = i`,
                                 `torch.manual_seed(1000 + i)` and `np.random.seed(1000 + i)` before each: the time indices numpy drew and the
                                 loss.  eta is NOT stored: it is the first draw after the seed, `torch.randn(eps.shape)` on the CPU generator.
    grad0_digest::*              digest of iteration 0's gradient of every parameter BEFORE clipping.  The test recomputes the gradients with
                                 oracle.ldt_oracle.score_forward + autograd in fp32 — asserted here to equal the reference's to <= 1e-10
                                 rel-MSE — and ties them to the captured ones through these digests.
    grad0::* / after1::* / after20::* / ema1::* / ema20::* / exp_avg1::*
                                 verbatim, for the tensors of at most 1024 elements (every bias, the label embedding): iteration 0's
                                 gradient, the weights and the EMA after iterations 1 and 20, exp_avg after iteration 1;  opt_shapes /
                                 opt_keys / opt1_step: the optimizer state's layout
    twin_after20_update_relmse, twin_ema20_update_relmse
                                 the bf16 twin's rel-MSE on the 20-step update (value - initial value) of those small tensors, concatenated
    lab_*                        the same setup with num_categorys = 3 and labels, one step: lab_init_digest::*, lab_cates, lab_idx, lab_loss,
                                 lab_grad0_digest::*
    twin_grad_relmse::<name>, twin_grad_relmse_all, twin_loss_dev (+ lab_twin_*)
                                 the distances of a bf16 twin from the fp32 reference — the yardsticks tests/test_gpu_train.py holds the HIP
                                 path to.  The twin is oracle.ldt_oracle.score_forward under torch.autocast("cpu", torch.bfloat16) (every
                                 GEMM's operands rounded to bf16) with autograd, clip_grad_norm_ and torch.optim.Adam, over the same 20
                                 iterations: per-tensor and concatenated rel-MSE of iteration 0's gradient, and
                                 twin_loss_dev = max_i |loss_twin_i - loss_ref_i| / loss_ref_i.

The script asserts that the oracle in fp32 reproduces the reference's gradients to <= 1e-10 rel-MSE, and prints the yardsticks.

    python tools/gen_score_train_golden.py
"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import ldt_oracle as O  # noqa: E402
from oracle import ref_import as R  # noqa: E402
from oracle.gen_checkpoint_golden import torch2_optimizer_compat  # noqa: E402
from oracle.gen_golden import save, tiny_cfg  # noqa: E402

ITERS, B = 20, 8
SMALL = 1024          # tensors of at most this many elements are stored verbatim next to their digest


def rel_mse(a, b):
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).sum() / (b ** 2).sum().clamp_min(1e-300))


def digest(t):
    t = torch.as_tensor(t).detach().double().reshape(-1)
    return torch.stack([t.sum(), (t * t).sum(), (t * torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64))).sum()])


def train_cfg(num_categorys=1):
    cfg = tiny_cfg(N=50)
    cfg.opt.lr, cfg.opt.warmup_iters, cfg.opt.ema_decay, cfg.opt.grad_norm_clip_value = 2e-3, 5, 0.98, 1.0
    cfg.opt.discrete, cfg.opt.loss_type = True, "l2"
    cfg.data.num_categorys = cfg.score.num_categorys = num_categorys
    return cfg


def oracle_loss(sd, cfg, sde, eps, idx, eta, cates=None, autocast=False):
    """Latent_SDE_Trainer.py:117-136 over oracle.score_forward (discrete times, l2)."""
    t = torch.linspace(1.0, cfg.sde.sample_time_eps, cfg.sde.train_N).index_select(0, idx)
    e2int_f, var = sde.e2int_f(t)[:, None, None], sde.var(t)[:, None, None]
    xt = eps * e2int_f + torch.sqrt(var) * eta
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        lab = None
        if cates is not None:
            e = sd["LabelEmbedding.label_emb.weight"][cates]
            lab = O.linear(sd, "LabelEmbedding.mlp.2", F.silu(O.linear(sd, "LabelEmbedding.mlp.0", e)))
        params = O.score_forward(sd, cfg.score, xt, t, label_emb=lab)
    return torch.square(eta - params.float()).mean()


def draw(i, shape, N):
    torch.manual_seed(1000 + i)
    np.random.seed(1000 + i)
    idx = torch.from_numpy(np.random.choice(np.arange(N), shape[0], replace=True))
    np.random.seed(1000 + i)                                  # the reference draws the same indices again
    return idx, torch.randn(shape)                            # eta: what randn_like(eps) will return after the same seed


def run(num_categorys, iters, out, tag=""):
    import trainer.Latent_SDE_Trainer as T
    from diffusion.diffusion_continuous import DiffusionVPSDE
    from model.Compressor.Network import Compressor
    from model.scorenet.score import Score
    cfg = train_cfg(num_categorys)
    torch.manual_seed(21)
    score, comp = Score(cfg.score), Compressor(cfg.compressor)
    comp.eval(); comp.init()
    init = copy.deepcopy(score.state_dict())
    import ldt_amd                                            # the test rebuilds the initial weights from the seed: same draws?
    torch.manual_seed(21)
    ours = ldt_amd.Score(cfg.score).state_dict()
    assert ours.keys() == init.keys() and all(torch.equal(ours[k], init[k]) for k in init), "ldt_amd.Score's default init differs from upstream's"
    names = [n for n, _ in score.named_parameters()]
    with R.quiet():
        tr = T.Trainer(cfg, score, comp, "cpu")
    torch2_optimizer_compat(tr.optimizer)
    g = torch.Generator().manual_seed(77)
    eps = torch.randn(B, cfg.score.z_scale, cfg.score.z_dim, generator=g) * 0.5
    cates = torch.tensor([0, 2, 1, 1, 0, 2, 2, 0]) if num_categorys > 1 else None
    grads = {}
    orig_clip = T.clip_grad_norm_

    def spy_clip(params, max_norm, *a, **k):
        params = list(params)
        if not grads:
            grads.update({n: p.grad.detach().clone() for n, p in zip(names, params)})
        return orig_clip(params, max_norm, *a, **k)

    T.clip_grad_norm_ = spy_clip
    idxs, losses = [], []
    try:
        for i in range(iters):
            idx, _ = draw(i, eps.shape, cfg.sde.train_N)
            tr.itr = i
            torch.manual_seed(1000 + i)
            loss = tr.update_score(eps, cates=cates, discrete=True)
            idxs.append(idx); losses.append(float(loss))
            if i + 1 in (1, iters) and not tag:
                params = list(score.parameters())
                st0 = tr.optimizer.state[params[0]]
                out["opt_keys"] = np.array(sorted(st0.keys()))
                out["opt%d_step" % (i + 1)] = float(st0["step"])
                out["opt_shapes"] = np.array([";".join("x".join(map(str, v.shape)) for v in (p, tr.optimizer.state[p]["exp_avg"],
                                              tr.optimizer.state[p]["exp_avg_sq"], tr.optimizer.state[p]["ema"])) for p in params])
                for n, p in zip(names, params):               # the small tensors' state after iterations 1 and 20, verbatim
                    if p.numel() <= SMALL:
                        st = tr.optimizer.state[p]
                        out["after%d::%s" % (i + 1, n)] = p.detach().clone()
                        out["ema%d::%s" % (i + 1, n)] = st["ema"].detach().clone()
                        if i == 0:
                            out["exp_avg1::" + n] = st["exp_avg"].detach().clone()
    finally:
        T.clip_grad_norm_ = orig_clip
    out.update({tag + "init_digest::" + n: digest(v) for n, v in init.items()})
    out.update({tag + "grad0_digest::" + n: digest(v) for n, v in grads.items()})
    out.update({tag + "grad0::" + n: v for n, v in grads.items() if v.numel() <= SMALL})
    out[tag + "param_names"] = np.array(names)
    out[tag + "idx"], out[tag + "loss"] = torch.stack(idxs), torch.tensor(losses, dtype=torch.float64)
    if cates is not None:
        out[tag + "cates"] = cates
    if not tag:
        out["eps"] = eps

    # the oracle in fp32 (must reproduce the reference's gradients) and the bf16 twin (the yardsticks)
    sde = DiffusionVPSDE(cfg.sde)
    for twin in (False, True):
        sd = {k: v.clone() for k, v in init.items()}
        leaves = [sd[n].requires_grad_(True) for n in names]
        opt = torch.optim.Adam(leaves, lr=cfg.opt.lr, betas=(cfg.opt.beta1, cfg.opt.beta2), weight_decay=cfg.opt.weight_decay)
        dev, ema = 0.0, None
        for i in range(iters if twin else 1):
            idx, eta = draw(i, eps.shape, cfg.sde.train_N)
            for grp in opt.param_groups:
                grp["lr"] = cfg.opt.lr * min(float(i + 1) / max(cfg.opt.warmup_iters, 1), 1.0) if i < cfg.opt.warmup_iters else grp["lr"]
            opt.zero_grad()
            loss = oracle_loss(sd, cfg, sde, eps, idx, eta, cates, autocast=twin)
            loss.backward()
            if i == 0:
                per = {n: rel_mse(p.grad, grads[n]) for n, p in zip(names, leaves)}
                allg = rel_mse(torch.cat([p.grad.reshape(-1) for p in leaves]), torch.cat([grads[n].reshape(-1) for n in names]))
                if not twin:
                    worst = max(max(per.values()), allg)
                    print("%sfp32 oracle vs reference: worst gradient rel-MSE %.3e, loss %.9f vs %.9f" % (tag, worst, float(loss), losses[0]))
                    assert worst <= 1e-10, "the oracle does not reproduce the reference's gradients"
                else:
                    out.update({tag + "twin_grad_relmse::" + n: v for n, v in per.items()})
                    out[tag + "twin_grad_relmse_all"] = allg
                    print("%stwin gradient rel-MSE: all %.3e, per tensor %.3e .. %.3e" % (tag, allg, min(per.values()), max(per.values())))
            dev = max(dev, abs(float(loss) - losses[i]) / losses[i])
            torch.nn.utils.clip_grad_norm_(leaves, cfg.opt.grad_norm_clip_value)
            opt.step()
            with torch.no_grad():                             # tools/utils.py:49-62
                ema = [p.detach().clone() for p in leaves] if ema is None else ema
                ema = [e * cfg.opt.ema_decay + (1. - cfg.opt.ema_decay) * p for e, p in zip(ema, leaves)]
        if twin and not tag:                                  # how far the twin's 20-step UPDATE of the small tensors is from the reference's
            small = [(n, p.detach(), e) for n, p, e in zip(names, leaves, ema) if p.numel() <= SMALL]
            upd = lambda vals: torch.cat([(v - init[n]).reshape(-1) for (n, _, _), v in zip(small, vals)])
            out["twin_after20_update_relmse"] = rel_mse(upd([p for _, p, _ in small]), upd([out["after20::" + n] for n, _, _ in small]))
            out["twin_ema20_update_relmse"] = rel_mse(upd([e for _, _, e in small]), upd([out["ema20::" + n] for n, _, _ in small]))
            print("twin 20-step update of the small tensors: weights rel-MSE %.3e, EMA %.3e" % (out["twin_after20_update_relmse"], out["twin_ema20_update_relmse"]))
        if twin:
            out[tag + "twin_loss_dev"] = dev
            print("%stwin_loss_dev over %d iterations: %.3e (losses %.4f -> %.4f)" % (tag, iters, dev, losses[0], losses[-1]))


def main():
    R.setup()
    out = {}
    run(1, ITERS, out)
    run(3, 1, out, tag="lab_")
    save("score_train_tiny", **out)


if __name__ == "__main__":
    main()
