"""Helpers of the conditioned whole-step tests (test_train_cond_host.py, test_gpu_train_cond.py) and of the tool that captures their
fixture (tools/gen_score_train_cond_golden.py -> tests/golden/score_train_cond.npz): the three model layouts, the training options, the
fixed latents and conditions, and the fp32 oracle gradients — with respect to the parameters and to the condition pair — tied to the
fixture's digests.

A condition is the embedded pair ConditionNet returns: (pts_condition (B, hidden, S) channels-first, img_condition (B, t_dim)).  The Scores
here are built with `condition: False` (no ConditionNet in the model): such a Score accepts the pair (score.py:129-133)."""
import copy
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HIDDEN, T_DIM, Z = 128, 128, 120
# Score hidden 128, t_dim 128, z 120 throughout; even blocks cross-attend to the S condition tokens
MODELS = {
    "x": dict(num_heads=2, num_blocks=3, B=3, T=40, S=24, num_categorys=1, iters=20),     # 64-wide heads; blocks 0 and 2 cross
    "y": dict(num_heads=16, num_blocks=2, B=4, T=32, S=32, num_categorys=1, iters=1),     # 8-wide heads
    "z": dict(num_heads=4, num_blocks=2, B=2, T=24, S=40, num_categorys=3, iters=1),      # 32-wide heads; a label AND a condition
}
CATES = {"z": torch.tensor([2, 0])}

_CACHE = {}


def apply_overrides(cfg, key):
    m = MODELS[key]
    cfg.score.hidden_size, cfg.score.t_dim, cfg.score.z_dim, cfg.score.condition = HIDDEN, T_DIM, Z, False
    cfg.score.num_heads, cfg.score.num_blocks, cfg.score.z_scale = m["num_heads"], m["num_blocks"], m["T"]
    return cfg


def set_train_options(cfg, key, **opt):
    cfg.opt.lr, cfg.opt.warmup_iters, cfg.opt.ema_decay, cfg.opt.grad_norm_clip_value = 2e-3, 5, 0.98, 1.0
    cfg.opt.discrete, cfg.opt.loss_type = True, "l2"
    cfg.data.num_categorys = cfg.score.num_categorys = MODELS[key]["num_categorys"]
    for k, v in opt.items():
        setattr(cfg.opt, k, v)
    return cfg


def train_cfg(tiny_cfg, key, **opt):
    return set_train_options(apply_overrides(copy.deepcopy(tiny_cfg), key), key, **opt)


def latents(key):
    m = MODELS[key]
    g = torch.Generator().manual_seed(77)
    return torch.randn(m["B"], m["T"], Z, generator=g) * 0.5


def conditions(key):
    """(pts_condition (B, hidden, S), img_condition (B, t_dim)): seeded randn x 0.5."""
    m = MODELS[key]
    g = torch.Generator().manual_seed(78)
    return torch.randn(m["B"], HIDDEN, m["S"], generator=g) * 0.5, torch.randn(m["B"], T_DIM, generator=g) * 0.5


def cates_of(key):
    return CATES.get(key)


def golden():
    if "g" not in _CACHE:
        z = np.load(os.path.join(GOLDEN, "score_train_cond.npz"))
        _CACHE["g"] = {k: (torch.from_numpy(np.asarray(z[k])) if z[k].dtype.kind in "fiu" else z[k]) for k in z.files}
    return _CACHE["g"]


def digest(t):
    t = torch.as_tensor(t).detach().double().cpu().reshape(-1)
    return torch.stack([t.sum(), (t * t).sum(), (t * torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64))).sum()])


def rel_mse(a, b):
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).sum() / (b ** 2).sum().clamp_min(1e-300))


def same_digest(t, want, tol=1e-9):
    got = digest(t)
    return float((got - want).abs().max()) <= tol * (float(want[1]) * torch.as_tensor(t).numel()) ** 0.5 + 1e-300


def inputs_of(key):
    """The fixture's latents and condition pair, drawn again from their seeds and checked against the stored digests."""
    g = golden()
    eps, (pts, img) = latents(key), conditions(key)
    for nm, t in (("eps", eps), ("pts", pts), ("img", img)):
        assert same_digest(t, g["%s_%s_digest" % (key, nm)]), "%s differs from the fixture's: %s" % (nm, key)
    return eps, pts, img


def initial_score(cfg, key):
    """ldt_amd.Score on the fixture's initial weights (seed 21), checked against init_digest::* -> (model, CPU copy of its state_dict)."""
    import ldt_amd
    g = golden()
    torch.manual_seed(21)
    score = ldt_amd.Score(cfg.score)
    init = {k: v.detach().clone() for k, v in score.state_dict().items()}
    for k, v in init.items():
        assert same_digest(v, g[key + "_init_digest::" + k]), "initial weights differ from the fixture's: " + k
    return score, init


def draw(key, i):
    """The time indices and the noise of the fixture's iteration i (eta is the first draw after the seed)."""
    m = MODELS[key]
    torch.manual_seed(1000 + i)
    return golden()[key + "_idx"][i], torch.randn(m["B"], m["T"], Z)


def oracle_loss(sd, cfg, eps, t, e2int_f, var, eta, pts, img, cates=None):
    """completion_trainer/Latent_SDE_Trainer.py:131-140 over oracle.score_forward (l2, weight 1), in the dtype of `eps`.
    pts (B, hidden, S) channels-first as the trainer receives it (the oracle takes it token-major); img (B, t_dim) or 0."""
    from oracle import ldt_oracle as O
    xt = eps * e2int_f[:, None, None] + torch.sqrt(var)[:, None, None] * eta
    lab = None
    if cates is not None:
        lab = O.linear(sd, "LabelEmbedding.mlp.2", F.silu(O.linear(sd, "LabelEmbedding.mlp.0", sd["LabelEmbedding.label_emb.weight"][cates])))
    d = eta - O.score_forward(sd, cfg.score, xt, t, label_emb=lab, condition=(pts.transpose(1, 2), img)).float()
    return (d * d).mean()


def oracle_grads(init, cfg, names, eps, t, e2int_f, var, eta, pts, img, cates=None, dtype=torch.float32, autocast=False):
    """-> ({parameter name: gradient}, d loss / d pts, d loss / d img (None when a label displaces it), loss) by autograd."""
    c = lambda v: v.detach().clone().to(dtype)
    sd = {k: c(v) for k, v in init.items()}
    leaves = [sd[n].requires_grad_(True) for n in names]
    pts, img = c(pts).requires_grad_(True), c(img).requires_grad_(True)
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        loss = oracle_loss(sd, cfg, c(eps), c(t), c(e2int_f), c(var), c(eta), pts, img, cates=cates)
    loss.float().backward()
    return {n: p.grad for n, p in zip(names, leaves)}, pts.grad, img.grad, float(loss.detach())


def reference_grads0(tiny_cfg, key):
    """Iteration 0's reference gradients: the fp32 oracle + autograd (asserted equal to the reference's to 1e-10 rel-MSE when the fixture
    was captured), tied to the captured ones through grad0_digest::* / dcond_*_digest and replaced by the verbatim copies where the
    fixture has them (the small parameters; the condition gradients).  Once per model
    -> (parameter gradients by name, names, d_pts (B, hidden, S), d_img (B, t_dim) or None, loss)."""
    if ("ref", key) not in _CACHE:
        import ldt_amd
        g = golden()
        cfg = train_cfg(tiny_cfg, key)
        score, init = initial_score(cfg, key)
        names = [n for n, _ in score.named_parameters()]
        assert names == [str(n) for n in g[key + "_param_names"]]
        sde = ldt_amd.DiffusionVPSDE(cfg.sde)
        idx, eta = draw(key, 0)
        eps, pts, img = inputs_of(key)
        t = torch.linspace(1.0, cfg.sde.sample_time_eps, cfg.sde.train_N).index_select(0, idx)
        grads, d_pts, d_img, loss = oracle_grads(init, cfg, names, eps, t, sde.e2int_f(t), sde.var(t), eta, pts, img, cates=cates_of(key))
        for n in names:                                        # the captured reference, by digest: [sum, sum of squares, projection]
            want, got = g[key + "_grad0_digest::" + n], digest(grads[n])
            scale = float(want[1].sqrt()) * grads[n].numel() ** 0.5
            assert abs(float(got[1] - want[1])) <= 1e-5 * float(want[1]) and float((got - want)[[0, 2]].abs().max()) <= 1e-5 * scale, n
        assert abs(loss - float(g[key + "_loss"][0])) <= 1e-6 * loss
        for n in names:                                        # the small tensors are stored verbatim: THOSE are the reference
            if key + "_grad0::" + n in g:
                assert rel_mse(grads[n], g[key + "_grad0::" + n]) <= 1e-10, n
                grads[n] = g[key + "_grad0::" + n]
        assert rel_mse(d_pts, g[key + "_dcond_pts"]) <= 1e-10                    # the reference's own condition gradients, verbatim
        d_pts = g[key + "_dcond_pts"]
        if cates_of(key) is None:
            assert rel_mse(d_img, g[key + "_dcond_img"]) <= 1e-10
            d_img = g[key + "_dcond_img"]
        else:                                                  # score.py:135: the label displaces the image condition — no gradient reaches it
            assert key + "_dcond_img" not in g and (d_img is None or float(d_img.abs().max()) == 0.0)
            d_img = None
        _CACHE[("ref", key)] = (grads, names, d_pts, d_img, loss)
    return _CACHE[("ref", key)]
