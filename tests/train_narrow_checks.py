"""Helpers of the whole-step tests at head widths 8, 16 and 32 (test_train_narrow_host.py, test_gpu_train_narrow.py) and of the tool that
captures their fixture (tools/gen_score_train_narrow_golden.py -> tests/golden/score_train_narrow.npz): the three model layouts, the
training options, the fixed latents, and the fp32 oracle gradients tied to the fixture's digests."""
import copy
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B = 8
# Score hidden 128, t_dim 128, 2 blocks, z 120 throughout.  (a): the hybrid config's head layout and token count
MODELS = {
    "a": dict(num_heads=16, z_scale=32, num_categorys=1, iters=20),
    "b": dict(num_heads=8, z_scale=40, num_categorys=3, iters=1),
    "c": dict(num_heads=4, z_scale=24, num_categorys=1, iters=1),
}
CATES = torch.tensor([0, 2, 1, 1, 0, 2, 2, 0])        # tools/gen_score_train_golden.py's labels

_CACHE = {}


def apply_overrides(cfg, key):
    m = MODELS[key]
    cfg.score.hidden_size, cfg.score.t_dim, cfg.score.num_blocks, cfg.score.z_dim = 128, 128, 2, 120
    cfg.score.num_heads, cfg.score.z_scale = m["num_heads"], m["z_scale"]
    return cfg


def train_cfg(tiny_cfg, key, **opt):
    cfg = apply_overrides(copy.deepcopy(tiny_cfg), key)
    cfg.opt.lr, cfg.opt.warmup_iters, cfg.opt.ema_decay, cfg.opt.grad_norm_clip_value = 2e-3, 5, 0.98, 1.0
    cfg.opt.discrete, cfg.opt.loss_type = True, "l2"
    cfg.data.num_categorys = cfg.score.num_categorys = MODELS[key]["num_categorys"]
    for k, v in opt.items():
        setattr(cfg.opt, k, v)
    return cfg


def latents(key):
    g = torch.Generator().manual_seed(77)
    return torch.randn(B, MODELS[key]["z_scale"], 120, generator=g) * 0.5


def golden():
    if "g" not in _CACHE:
        z = np.load(os.path.join(GOLDEN, "score_train_narrow.npz"))
        _CACHE["g"] = {k: (torch.from_numpy(np.asarray(z[k])) if z[k].dtype.kind in "fiu" else z[k]) for k in z.files}
    return _CACHE["g"]


def digest(t):
    t = torch.as_tensor(t).detach().double().cpu().reshape(-1)
    return torch.stack([t.sum(), (t * t).sum(), (t * torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64))).sum()])


def rel_mse(a, b):
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).sum() / (b ** 2).sum().clamp_min(1e-300))


def eps_of(key):
    """The fixture's latents: stored for (a), drawn again and checked against the digest for (b) and (c)."""
    g = golden()
    if key + "_eps" in g:
        return g[key + "_eps"]
    eps = latents(key)
    want, got = g[key + "_eps_digest"], digest(eps)
    assert float((got - want).abs().max()) <= 1e-9 * (float(want[1]) * eps.numel()) ** 0.5, "latents differ from the fixture's: " + key
    return eps


def cates_of(key):
    return golden()[key + "_cates"] if MODELS[key]["num_categorys"] > 1 else None


def initial_score(cfg, key):
    """ldt_amd.Score on the fixture's initial weights (seed 21), checked against init_digest::* -> (model, CPU copy of its state_dict)."""
    import ldt_amd
    g = golden()
    torch.manual_seed(21)
    score = ldt_amd.Score(cfg.score)
    init = {k: v.detach().clone() for k, v in score.state_dict().items()}
    for k, v in init.items():
        want, got = g[key + "_init_digest::" + k], digest(v)       # (float64 sums: the summation order differs between hosts)
        assert float((got - want).abs().max()) <= 1e-9 * (float(want[1]) * v.numel()) ** 0.5 + 1e-300, "initial weights differ from the fixture's: " + k
    return score, init


def draw(key, i):
    """The time indices and the noise of the fixture's iteration i (eta is the first draw after the seed)."""
    torch.manual_seed(1000 + i)
    return golden()[key + "_idx"][i], torch.randn(B, MODELS[key]["z_scale"], 120)


def oracle_loss(sd, cfg, eps, t, e2int_f, var, eta, cates=None):
    """Latent_SDE_Trainer.py:127-136 over oracle.score_forward (l2, weight 1), in the dtype of `eps`."""
    from oracle import ldt_oracle as O
    xt = eps * e2int_f[:, None, None] + torch.sqrt(var)[:, None, None] * eta
    lab = None
    if cates is not None:
        lab = O.linear(sd, "LabelEmbedding.mlp.2", F.silu(O.linear(sd, "LabelEmbedding.mlp.0", sd["LabelEmbedding.label_emb.weight"][cates])))
    d = eta - O.score_forward(sd, cfg.score, xt, t, label_emb=lab)
    return (d * d).mean()


def reference_grads0(tiny_cfg, key):
    """Iteration 0's reference gradients: the fp32 oracle + autograd (asserted equal to the reference's to 1e-10 rel-MSE when the fixture
    was captured), tied to the captured ones through grad0_digest::* and replaced by the verbatim copies where the fixture has them.
    Computed once per model -> (gradients by name, names, loss)."""
    if ("ref", key) not in _CACHE:
        import ldt_amd
        g = golden()
        cfg = train_cfg(tiny_cfg, key)
        score, init = initial_score(cfg, key)
        names = [n for n, _ in score.named_parameters()]
        assert names == [str(n) for n in g[key + "_param_names"]]
        sde = ldt_amd.DiffusionVPSDE(cfg.sde)
        idx, eta = draw(key, 0)
        t = torch.linspace(1.0, cfg.sde.sample_time_eps, cfg.sde.train_N).index_select(0, idx)
        sd = {k: v.detach().clone() for k, v in init.items()}
        leaves = [sd[n].requires_grad_(True) for n in names]
        loss = oracle_loss(sd, cfg, eps_of(key), t, sde.e2int_f(t), sde.var(t), eta, cates=cates_of(key))
        loss.backward()
        loss = float(loss.detach())
        grads = {n: p.grad for n, p in zip(names, leaves)}
        for n in names:                                        # the captured reference, by digest: [sum, sum of squares, projection]
            want, got = g[key + "_grad0_digest::" + n], digest(grads[n])
            scale = float(want[1].sqrt()) * grads[n].numel() ** 0.5
            assert abs(float(got[1] - want[1])) <= 1e-5 * float(want[1]) and float((got - want)[[0, 2]].abs().max()) <= 1e-5 * scale, n
        assert abs(loss - float(g[key + "_loss"][0])) <= 1e-6 * loss
        for n in names:                                        # the small tensors are stored verbatim: THOSE are the reference
            if key + "_grad0::" + n in g:
                assert rel_mse(grads[n], g[key + "_grad0::" + n]) <= 1e-10, n
                grads[n] = g[key + "_grad0::" + n]
        _CACHE[("ref", key)] = (grads, names, loss)
    return _CACHE[("ref", key)]
