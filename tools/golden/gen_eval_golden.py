"""TEST INFRASTRUCTURE ONLY — writes tests/golden/eval_tiny.npz: what the reference computes on the held-out-evaluation path.

Runs only where the upstream reference can be imported (through oracle/ref_import.py, on CPU); the fixture is data, the reference
does not travel.  On the tiny config (tests/golden/tiny_cfg.json) with the weights the other fixtures carry (Score:
score_tiny.npz, Compressor: trainer_sample_tiny.npz) it captures

  * the reference `Compressor.forward` on the cloud and the recorded posterior noise of compressor_fwd_tiny.npz: `kls`,
    `all_logqz` (stored token-major, [level, B, tokens, z]), `all_eps`, `set` — and checks that `all_eps` is the tensor that
    fixture already holds;
  * the lines of `Trainer.val_loss` (trainer/Latent_SDE_Trainer.py:63-92) composed from the reference `Score` and `DiffusionVPSDE`
    in the method's order (the method itself hard-codes "cuda"): idx, t, e2int_f, var, eta, xt, params, and the loss for
    cfg.opt.loss_type "l1" and squared;
  * `inv_var` / `var_vpsde` / `inv_var_vpsde` / `var_N` / `inv_var_N` / `cross_entropy_const` / `sample_q` of the four SDE
    families at a few times.

    python tools/golden/gen_eval_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_import as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FAMILIES = {                                     # the constants of tests/golden/sde_types.npz
    "vpsde": dict(),
    "sub_vpsde": dict(),
    "vesde": dict(sigma2_min=0.01, sigma2_max=4.0, sigma2_0=0.01),
    "geometric_sde": dict(sigma2_min=3e-5, sigma2_max=0.999, sigma2_0=0.0),
}
VAL_NP_SEED, VAL_ETA_SEED = 2024, 99


def tiny_cfg():
    with open(os.path.join(GOLDEN, "tiny_cfg.json")) as f:
        return R.dict2ns(json.load(f))


def weights(npz, prefix):
    return {k[len(prefix):]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(prefix)}


def main():
    R.setup()
    from model.scorenet.score import Score
    from model.Compressor.Network import Compressor
    from diffusion.diffusion_continuous import DiffusionVPSDE, make_diffusion
    torch.set_grad_enabled(False)
    cfg = tiny_cfg()
    out = {}

    # ---- Compressor.forward with the recorded posterior noise: kls / all_logqz ------------------------------------
    comp = Compressor(cfg.compressor).eval()
    comp.load_state_dict(weights(np.load(os.path.join(GOLDEN, "trainer_sample_tiny.npz")), "c::"), strict=True)
    comp.init()
    fwd = np.load(os.path.join(GOLDEN, "compressor_fwd_tiny.npz"))
    pts = torch.from_numpy(fwd["pts"])
    noise = iter([torch.from_numpy(n).transpose(1, 2).contiguous() for n in fwd["post_noise"]])   # drawn as (B, z, tokens)
    o_randn = torch.randn
    torch.randn = lambda *a, **k: next(noise)
    try:
        res = comp(pts)
    finally:
        torch.randn = o_randn
    assert torch.equal(res["all_eps"], torch.from_numpy(fwd["all_eps"])), "not the forward compressor_fwd_tiny.npz recorded"
    out["kls"] = torch.stack([k.transpose(1, 2) for k in res["kls"]], 0)
    out["all_logqz"] = torch.stack([k.transpose(1, 2) for k in res["all_logqz"]], 0)
    out["all_eps"], out["set"] = res["all_eps"], res["set"]
    out["kl_loss"] = torch.cat(res["kls"], dim=1).mean()

    # ---- Trainer.val_loss, line by line ------------------------------------------------------------------------------
    score = Score(cfg.score).eval()
    score.load_state_dict(weights(np.load(os.path.join(GOLDEN, "score_tiny.npz")), "w::"), strict=True)
    with R.quiet():
        sde = DiffusionVPSDE(cfg.sde)
    eps = res["all_eps"]
    size, N = eps.shape[0], cfg.sde.train_N
    timesteps = torch.linspace(1.0, cfg.sde.sample_time_eps, N)
    np.random.seed(VAL_NP_SEED)
    idx = torch.from_numpy(np.random.choice(np.arange(N), size, replace=True))
    t = timesteps.index_select(0, idx)
    e2int_f = sde.e2int_f(t)[:, None, None]
    var = sde.var(t)[:, None, None]
    weight_p = torch.ones(1)
    torch.manual_seed(VAL_ETA_SEED)
    eta = torch.randn_like(eps)
    xt = eps * e2int_f + torch.sqrt(var) * eta
    params = score(xt, t, condition=None, label=None)
    out.update({"val/np_seed": VAL_NP_SEED, "val/idx": idx, "val/t": t, "val/e2int_f": e2int_f.reshape(-1), "val/var": var.reshape(-1),
                "val/eta": eta, "val/xt": xt, "val/params": params,
                "val/loss_l1": (torch.abs(eta - params) * weight_p).mean(),
                "val/loss_l2": (torch.square(eta - params) * weight_p).mean()})

    # ---- closed-form schedule methods ----------------------------------------------------------------------------------
    probe = torch.tensor([1.0, 0.73519, 0.5, 0.1, 1e-2, 1e-3], dtype=torch.float32)
    out["sde/probe_t"] = probe
    g = torch.Generator().manual_seed(3)
    x_init, q_noise = torch.randn(probe.numel(), 5, generator=g), torch.randn(probe.numel(), 5, generator=g)
    out["sde/x_init"], out["sde/noise"] = x_init, q_noise
    for name, extra in FAMILIES.items():
        c = tiny_cfg()
        c.sde.sde_type = name
        for k, v in extra.items():
            setattr(c.sde, k, v)
            out["sde/%s/%s" % (name, k)] = v
        with R.quiet():
            fam = make_diffusion(c.sde)
        v = fam.var(probe)
        out["sde/%s/var" % name] = v
        if name != "sub_vpsde":                                     # (raises NotImplementedError upstream)
            out["sde/%s/inv_var" % name] = fam.inv_var(v)
        if name == "sub_vpsde":
            out["sde/%s/var_vpsde" % name] = fam.var_vpsde(probe)
            out["sde/%s/inv_var_vpsde" % name] = fam.inv_var_vpsde(fam.var_vpsde(probe))
        if name == "vesde":
            out["sde/%s/var_N" % name] = fam.var_N(probe)
            out["sde/%s/inv_var_N" % name] = fam.inv_var_N(fam.var_N(probe))
        out["sde/%s/cross_entropy_const" % name] = fam.cross_entropy_const(1e-3)
        out["sde/%s/sample_q" % name] = fam.sample_q(x_init, q_noise, v[:, None], fam.e2int_f(probe)[:, None])

    path = os.path.join(GOLDEN, "eval_tiny.npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()})
    print("wrote %s %.1f KB" % (path, os.path.getsize(path) / 1024))
    for k in ("kl_loss", "val/loss_l1", "val/loss_l2", "val/idx", "val/t"):
        print(k, out[k])


if __name__ == "__main__":
    main()
