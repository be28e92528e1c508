"""CPU: the held-out-evaluation surface against tests/golden/eval_tiny.npz (captured from the reference by
tools/golden/gen_eval_golden.py) — the arithmetic of `Trainer.val_loss` and of the per-level KL / log q(z) restated in plain
fp32 torch from the formulas (the yardstick tests/test_gpu_eval.py then holds the HIP kernels to), the closed-form schedule
methods, and the public names / parameter lists of the new classes."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden, rel_mse

LOG_SQRT_2PI = 0.9189385332


def eval_golden():
    z = np.load(os.path.join(GOLDEN, "eval_tiny.npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def kl_terms(eps, mu, logvar):
    """Network.py:12-19,221-224 in the dtype of the inputs: (logqz, kl)."""
    logqz = -0.5 * torch.square(eps - mu) / torch.exp(logvar) - 0.5 * logvar - LOG_SQRT_2PI
    logpz = -0.5 * torch.square(eps) - LOG_SQRT_2PI
    return logqz, logqz - logpz


def val_loss_lines(sde, eps, t, eta, score_fn, loss_type):
    """Latent_SDE_Trainer.py:77-87 in fp32 torch: -> (xt, params, loss)."""
    e2int_f = sde.e2int_f(t)[:, None, None]
    var = sde.var(t)[:, None, None]
    xt = eps * e2int_f + torch.sqrt(var) * eta
    params = score_fn(xt, t)
    distance = torch.abs(eta - params) if loss_type == "l1" else torch.square(eta - params)
    return xt, params, (distance * torch.ones(1)).mean()


def test_kl_and_logqz_restatement_matches_the_reference():
    g = eval_golden()
    a, _ = load_golden("compressor_fwd_tiny")                   # mu / logvar / all_eps of the same forward, token-major
    L, z = a["mu"].shape[0], a["mu"].shape[-1]
    assert torch.equal(g["all_eps"], a["all_eps"])
    for j in range(L):
        eps = a["all_eps"][..., z * j: z * (j + 1)]
        logqz, kl = kl_terms(eps, a["mu"][j], a["logvar"][j])
        assert logqz.dtype == torch.float32
        assert rel_mse(logqz, g["all_logqz"][j]) <= 1e-10
        assert rel_mse(kl, g["kls"][j]) <= 1e-10
    # the way the reference trainers reduce them (Compressor_Trainer.py:48-49): channels-first list -> cat(dim=1).mean()
    kls_cf = [g["kls"][j].transpose(1, 2) for j in range(L)]
    assert abs(float(torch.cat(kls_cf, dim=1).mean()) - float(g["kl_loss"])) <= 1e-7


def test_val_loss_restatement_matches_the_reference(tiny_cfg):
    import ldt_amd
    from oracle import ldt_oracle as O
    g = eval_golden()
    _, ssd = load_golden("score_tiny")
    sde = ldt_amd.DiffusionVPSDE(tiny_cfg.sde)
    N = tiny_cfg.sde.train_N
    np.random.seed(int(g["val/np_seed"]))
    idx = torch.from_numpy(np.random.choice(np.arange(N), g["all_eps"].shape[0], replace=True))
    assert torch.equal(idx, g["val/idx"])                       # the numpy draw upstream makes
    t = torch.linspace(1.0, tiny_cfg.sde.sample_time_eps, N).index_select(0, idx)
    assert torch.equal(t, g["val/t"])
    assert float((sde.e2int_f(t) - g["val/e2int_f"]).abs().max()) <= 1e-6 and float((sde.var(t) - g["val/var"]).abs().max()) <= 1e-6
    score_fn = lambda x, tt: O.score_forward(ssd["w"], tiny_cfg.score, x, tt)
    for loss_type in ("l1", "l2"):
        xt, params, loss = val_loss_lines(sde, g["all_eps"], t, g["val/eta"], score_fn, loss_type)
        assert rel_mse(xt, g["val/xt"]) <= 1e-10
        assert rel_mse(params, g["val/params"]) <= 1e-10
        assert rel_mse(loss, g["val/loss_" + loss_type]) <= 1e-10
    assert float(g["val/loss_l1"]) != float(g["val/loss_l2"])


FAMILIES = ("vpsde", "sub_vpsde", "vesde", "geometric_sde")


def _family(tiny_cfg, g, name):
    import copy
    import ldt_amd
    c = copy.deepcopy(tiny_cfg.sde)
    c.sde_type = name
    for k in ("sigma2_min", "sigma2_max", "sigma2_0"):
        if "sde/%s/%s" % (name, k) in g:
            setattr(c, k, float(g["sde/%s/%s" % (name, k)]))
    return ldt_amd.make_diffusion(c)


@pytest.mark.parametrize("name", FAMILIES)
def test_schedule_closed_forms_match_the_reference(tiny_cfg, name):
    g = eval_golden()
    sde = _family(tiny_cfg, g, name)
    t = g["sde/probe_t"]
    near = lambda a, b: float((a - b).abs().max()) <= 1e-6
    v = sde.var(t)
    assert v.dtype == torch.float32 and near(v, g["sde/%s/var" % name])
    if name == "sub_vpsde":                                      # no closed form upstream either (diffusion_continuous.py:715-716)
        with pytest.raises(NotImplementedError):
            sde.inv_var(v)
        assert near(sde.var_vpsde(t), g["sde/sub_vpsde/var_vpsde"])
        assert near(sde.inv_var_vpsde(sde.var_vpsde(t)), g["sde/sub_vpsde/inv_var_vpsde"])
        assert float((sde.inv_var_vpsde(sde.var_vpsde(t.double())) - t.double()).abs().max()) <= 1e-6
    else:
        assert near(sde.inv_var(v), g["sde/%s/inv_var" % name])
        assert float((sde.inv_var(sde.var(t.double())) - t.double()).abs().max()) <= 1e-6      # inv_var(var(t)) = t
    if name == "vesde":
        assert near(sde.var_N(t), g["sde/vesde/var_N"])
        assert near(sde.inv_var_N(sde.var_N(t)), g["sde/vesde/inv_var_N"])
        assert float((sde.inv_var_N(sde.var_N(t.double())) - t.double()).abs().max()) <= 1e-6
    assert near(sde.cross_entropy_const(1e-3), g["sde/%s/cross_entropy_const" % name])
    xq = sde.sample_q(g["sde/x_init"], g["sde/noise"], v[:, None], sde.e2int_f(t)[:, None])   # host tensors: the host expression
    assert near(xq, g["sde/%s/sample_q" % name])


def _params(fn):
    return [(p.name, None if p.default is inspect.Parameter.empty else p.default) for p in inspect.signature(fn).parameters.values()
            if p.kind is not inspect.Parameter.KEYWORD_ONLY]


# the public methods of trainer/Compressor_Trainer.py and completion_trainer/Compressor_Trainer.py: (name, default) per parameter
UPSTREAM_COMPRESSOR_TRAINER = {
    "__init__": [("self", None), ("cfg", None), ("model", None), ("device", None)],
    "update": [("self", None), ("data", None)],
    "compute_loss": [("self", None), ("target_set", None), ("label", None)],
    "sample": [("self", None), ("num_samples", None), ("num_points", None), ("given_eps", None)],
    "valsample": [("self", None), ("test_loader", None), ("sample_points", None), ("vis", False)],
    "reconstrustion": [("self", None), ("test_loader", None), ("val_cate", 0)],
    "resume": [("self", None), ("epoch", None), ("finetune", False), ("strict", False), ("load_optim", True)],
}
UPSTREAM_COMPLETION_COMPRESSOR_TRAINER = {
    "__init__": [("self", None), ("cfg", None), ("model", None), ("device", None)],
    "update": [("self", None), ("data", None)],
    "compute_loss": [("self", None), ("target_set", None)],
    "sample": [("self", None), ("num_samples", None), ("num_points", None), ("given_eps", None)],
    "reconstrustion": [("self", None), ("test_loader", None)],
    "resume": [("self", None), ("epoch", None), ("finetune", False), ("strict", False), ("load_optim", True)],
    "load_pretrain": [("self", None)],
}


def test_public_surface_has_the_upstream_names_and_parameters():
    import ldt_amd
    for cls, want in ((ldt_amd.CompressorTrainer, UPSTREAM_COMPRESSOR_TRAINER),
                      (ldt_amd.CompletionCompressorTrainer, UPSTREAM_COMPLETION_COMPRESSOR_TRAINER)):
        for name, params in want.items():
            assert _params(getattr(cls, name)) == params, (cls.__name__, name)
    assert _params(ldt_amd.Trainer.val_loss) == [("self", None), ("data", None), ("condition", None)]      # Latent_SDE_Trainer.py:63
    kw = [p.name for p in inspect.signature(ldt_amd.Trainer.val_loss).parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert kw == ["t_index", "eta", "seed"]
    assert _params(ldt_amd.DiffusionBase.sample_q) == [("self", None), ("x_init", None), ("noise", None), ("var_t", None), ("m_t", None)]
    assert inspect.signature(ldt_amd.Compressor.forward).parameters["want_kl"].default is False
    for fn in ("reparam_kl", "diffuse_q", "dsm_loss"):
        assert callable(getattr(ldt_amd.ops, fn))


def test_training_entry_points_are_refused_with_a_reason(tiny_cfg):
    import ldt_amd
    comp = ldt_amd.Compressor(tiny_cfg.compressor)
    for cls in (ldt_amd.CompressorTrainer, ldt_amd.CompletionCompressorTrainer):
        tr = cls(tiny_cfg, comp, "cpu")
        assert (tr.epoch, tr.itr, tr.time) == (1, 0, 0)
        with pytest.raises(NotImplementedError, match="not on this path"):
            tr.update({})
        with pytest.raises(NotImplementedError, match="EMD"):
            tr.compute_loss(*([None] * (len(_params(cls.compute_loss)) - 1)))
        with pytest.raises(NotImplementedError, match="mitsuba"):
            tr.valsample([], 64, vis=True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):                 # no quiet fall-back to eager PyTorch
            tr.eval_losses(torch.zeros(2, 64, 3))


def test_header_binding_and_abi_number_agree():
    from ldt_amd import _lib
    src = open(os.path.join(ROOT, "include", "ldt_hip.h")).read()
    assert int(re.search(r"#define LDT_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 26
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("ldt_reparam_kl", "ldt_diffuse_q", "ldt_dsm_loss", "ldt_gemm_route"):
        m = re.search(r"\bint %s\s*\((.*?)\)\s*;" % name, decl, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name        # one ctypes entry per declared parameter


def test_new_entry_points_return_argument_errors():
    """Null pointers and impossible shapes come back as status codes with a message (no launch, so no GPU needed)."""
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib
    lib = _lib.lib()
    assert lib.ldt_reparam_kl(None, None, None, 0, None, None, None, None, None, 1, 1, 4, 0., 1., None) == -1
    assert b"null" in lib.ldt_last_error()
    assert lib.ldt_reparam_kl(16, 16, 16, 4, None, None, None, None, None, 6, 4, 4, 0., 1., None) == -2      # rows % rows_per_sample
    assert lib.ldt_reparam_kl(16, 16, 16, 4, 16, None, None, None, None, 8, 4, 4, 0., 1., None) == -1         # mu without logvar
    assert lib.ldt_diffuse_q(None, None, None, None, None, None, 1, 4, 0, 0, None) == -1
    assert lib.ldt_diffuse_q(16, None, 16, 16, 16, None, 1, 4, 0, 0, None) == -1 and b"eta" in lib.ldt_last_error()
    assert lib.ldt_diffuse_q(16, 16, 16, 16, 16, None, 1, 6, 0, 0, None) == -2                                  # per_sample % 4
    assert lib.ldt_diffuse_q(16, 20, 16, 16, 16, None, 1, 8, 0, 0, None) == -3                                  # alignment
    assert lib.ldt_dsm_loss(16, 16, None, 1, 8, 0, None, None, None) == -1
    assert lib.ldt_dsm_loss(16, 16, None, 0, 8, 0, 16, None, None) == -2
