"""CPU: the hybrid trainer's evaluation surface — `DiffusionBase.iw_quantities` against tests/golden/iw_quantities.npz, the JSD helpers of
`ldt_amd.metrics` against tests/golden/jsd.npz (both captured from the reference by tools/golden/gen_hybrid_eval_golden.py), the public
names / parameter lists of `HybridTrainer`, its refusals, and the argument errors of the two new C-ABI entry points."""
import copy
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

FAMILIES = ("vpsde", "sub_vpsde", "vesde", "geometric_sde")
MODES = ("ll_uniform", "ll_iw", "drop_all_uniform", "drop_all_iw", "drop_sigma2t_iw", "drop_sigma2t_uniform", "rescale_iw")
OUTPUTS = ("t", "var_t", "m_t", "obj_weight_t", "obj_weight_t_ll", "g2_t")


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: np.asarray(z[k]) for k in z.files}


def family(tiny_cfg, g, name):
    import ldt_amd
    c = copy.deepcopy(tiny_cfg.sde)
    c.sde_type = name
    for k in ("sigma2_min", "sigma2_max", "sigma2_0"):
        if "%s/%s" % (name, k) in g:
            setattr(c, k, float(g["%s/%s" % (name, k)]))
    return ldt_amd.make_diffusion(c)


# ------------------------------------------------------------------------------------------------ iw_quantities
@pytest.mark.parametrize("name", FAMILIES)
def test_iw_quantities_match_the_reference(tiny_cfg, name):
    """Every mode of the family on the stored rho.  The arithmetic is the reference's fp32 chain, so on the capturing host the outputs are
    equal; another host's vector maths may differ by an ulp per operation and some modes are ill conditioned near var -> 1.  The bar per
    output array is therefore the reference's own fp32-vs-float64 error, which carries the conditioning:
        max|mine - ref| <= 4 x max|ref - ref_f64|,   with a floor of one fp32 ulp of max|ref|."""
    g = golden("iw_quantities")
    sde = family(tiny_cfg, g, name)
    rho = torch.from_numpy(g["rho"])
    assert rho.numel() >= 64 and float(rho[0]) == 0.0 and float(rho[1]) == 1.0 - 2.0 ** -24
    time_eps = float(g["%s/time_eps" % name])
    worst = 0.0
    for mode in MODES:
        if "%s/%s/raises" % (name, mode) in g:                   # drop_all_iw on the geometric SDE: upstream's assert
            with pytest.raises(AssertionError):
                sde.iw_quantities(rho.numel(), time_eps, mode, name == "sub_vpsde", rho=rho)
            continue
        six = sde.iw_quantities(rho.numel(), time_eps, mode, name == "sub_vpsde", rho=rho)
        assert len(six) == 6
        for key, mine in zip(OUTPUTS, six):
            ref, ref64 = g["%s/%s/%s" % (name, mode, key)], g["%s/%s/%s_f64" % (name, mode, key)]
            assert mine.dtype == torch.float32 and mine.device.type == "cpu" and tuple(mine.shape) == ref.shape, (mode, key)
            want_shape = (rho.numel(),) if key == "t" else ((1, 1) if (key, mode) == ("obj_weight_t", "drop_all_uniform") else (rho.numel(), 1))
            assert tuple(mine.shape) == want_shape, (mode, key)
            err = float(np.abs(mine.numpy().astype(np.float64) - ref.astype(np.float64)).max())
            own = float(np.abs(ref.astype(np.float64) - ref64).max())
            bar = max(4.0 * own, float(np.spacing(np.float32(np.abs(ref).max()))))
            ratio = err / bar
            worst = max(worst, ratio)
            print("iw_quantities %-13s %-20s %-15s max|mine-ref| %.3e, reference's own fp32 error %.3e, bar %.3e, ratio %.3f"
                  % (name, mode, key, err, own, bar, ratio))
            assert err <= bar, (name, mode, key, err, bar)
    print("iw_quantities %s: largest error / bar over all modes and outputs: %.3f" % (name, worst))


def test_iw_quantities_errors_default_draw_and_constants(tiny_cfg):
    import ldt_amd
    g = golden("iw_quantities")
    vp, sub, ve = (family(tiny_cfg, g, n) for n in ("vpsde", "sub_vpsde", "vesde"))
    for sde in (vp, sub, ve):
        with pytest.raises(ValueError, match="Unrecognized importance sampling type"):
            sde.iw_quantities(4, 0.01, "no_such_mode", True)
    for mode in ("ll_iw", "drop_all_iw", "drop_sigma2t_iw"):     # the sub-VP IW modes exist only through the analogous VP-SDE
        with pytest.raises(NotImplementedError):
            sub.iw_quantities(4, 0.01, mode, False)
        assert sub.iw_quantities(4, 0.01, mode, True)[0].shape == (4,)
    assert sub.iw_quantities(4, 0.01, "ll_uniform", False)[0].shape == (4,)       # (the uniform modes do not need the flag)
    with pytest.raises(AssertionError, match="only implemented for the regular VPSDE"):
        family(tiny_cfg, g, "geometric_sde").iw_quantities(4, 0.01, "drop_all_iw", False)
    other = copy.copy(vp)
    other.sde_type = "something_else"
    with pytest.raises(NotImplementedError):
        other.iw_quantities(4, 0.01, "ll_uniform", False)
    with pytest.raises(ValueError, match="rho"):
        vp.iw_quantities(4, 0.01, "ll_uniform", False, rho=torch.zeros(3))
    # the default draw is ONE torch.rand(size) on the CPU generator
    torch.manual_seed(5)
    rho = torch.rand(6)
    after = torch.get_rng_state()
    torch.manual_seed(5)
    t = vp.iw_quantities(6, 0.01, "ll_iw", False)[0]
    assert torch.equal(torch.get_rng_state(), after)
    assert torch.equal(t, vp.iw_quantities(6, 0.01, "ll_iw", False, rho=rho)[0])
    assert float(t.min()) >= 0.01 - 1e-6 and float(t.max()) <= 1.0 + 1e-6
    # the auxiliary constants (diffusion_continuous.py:637-645), against float64
    from math import erf, exp, pi, sqrt
    b0, b1, s0, te = vp.beta_start, vp.beta_end, vp.sigma2_0, vp.time_eps
    dbh, bf = 0.5 * (b1 - b0), b0 / (b1 - b0)
    aq = (1.0 - s0) * exp(0.5 * bf) * sqrt(0.25 * pi / dbh)
    ce = erf(sqrt(dbh) * (te + bf))
    n2 = erf(sqrt(dbh) * (1.0 + bf)) - ce
    for sde in (vp, sub):
        for name, want in (("delta_beta_half", dbh), ("beta_frac", bf), ("const_aq", aq), ("const_erf", ce), ("const_norm", aq * n2),
                           ("const_norm_2", n2)):
            got = getattr(sde, name)
            assert torch.is_tensor(got) and got.dtype == torch.float32 and got.dim() == 0, name
            assert abs(float(got) - want) <= 4e-7 * max(abs(want), 1.0), (name, float(got), want)
    assert isinstance(ldt_amd.diffusion.IW_MODES, tuple) and set(ldt_amd.diffusion.IW_MODES) == set(MODES)


# ------------------------------------------------------------------------------------------------ HybridTrainer
def _params(fn):
    return [(p.name, None if p.default is inspect.Parameter.empty else p.default) for p in inspect.signature(fn).parameters.values()
            if p.kind is not inspect.Parameter.KEYWORD_ONLY]


def _kwonly(fn):
    return [p.name for p in inspect.signature(fn).parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY]


# the methods of trainer/Hybrid_Trainer.py: (name, default) per parameter (*args / **kwargs by name)
UPSTREAM_HYBRID_TRAINER = {
    "__init__": [("self", None), ("cfg", None), ("model", None), ("compressor", None), ("device", None)],
    "score_fn": [("self", None), ("t", None), ("x", None), ("label", None), ("condition", None)],
    "update": [("self", None), ("data", None), ("condition", None), ("train_individual", True)],
    "update_score": [("self", None), ("eps", None), ("condition", None), ("cates", None)],
    "clc_compressor": [("self", None), ("point", None), ("cates", None), ("condition", None), ("discrete", False), ("train_score", True)],
    "sample": [("self", None), ("num_samples", None), ("label", None), ("condition", None)],
    "valsample": [("self", None), ("test_loader", None), ("val_cate", 0), ("vis", False)],
    "valrecon": [("self", None), ("test_loader", None), ("val_cate", 0), ("args", None), ("kwargs", None)],
    "save": [("self", None), ("kwargs", None)],
    "resume": [("self", None), ("epoch", None), ("strict", False), ("load_optim", True), ("finetune", False), ("kwargs", None)],
    "load_pretrain": [("self", None)],
}
KEYWORD_EXTENSIONS = {
    "sample": ["num_points", "x0", "noise", "seed", "use_graph", "trajectory"],
    "resume": ["pretrain"],
    "val_nelbo": ["discrete", "rho", "t_index", "eta", "post_noise", "seed"],
}


def test_hybrid_trainer_has_the_upstream_names_and_parameters():
    import ldt_amd
    cls = ldt_amd.HybridTrainer
    for name, params in UPSTREAM_HYBRID_TRAINER.items():
        assert _params(getattr(cls, name)) == params, name
        assert _kwonly(getattr(cls, name)) == KEYWORD_EXTENSIONS.get(name, []), name
    assert inspect.signature(cls.valrecon).parameters["args"].kind is inspect.Parameter.VAR_POSITIONAL
    assert inspect.signature(cls.resume).parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert _params(cls.val_nelbo) == [("self", None), ("data", None), ("condition", None)]
    assert _kwonly(cls.val_nelbo) == KEYWORD_EXTENSIONS["val_nelbo"]
    assert _params(ldt_amd.DiffusionBase.iw_quantities) == [("self", None), ("size", None), ("time_eps", None), ("iw_sample_mode", None),
                                                            ("iw_subvp_like_vp_sde", None)]
    assert _kwonly(ldt_amd.DiffusionBase.iw_quantities) == ["rho", "device"]
    assert "HybridTrainer" in ldt_amd.__all__
    for fn in ("nelbo_terms", "occupancy_grid"):
        assert callable(getattr(ldt_amd.ops, fn))
    m = ldt_amd.metrics
    assert _params(m.unit_cube_grid_point_cloud) == [("resolution", None), ("clip_sphere", False)]
    assert _params(m.entropy_of_occupancy_grid) == [("pclouds", None), ("grid_resolution", None), ("in_sphere", False), ("verbose", False)]
    assert _params(m.jensen_shannon_divergence) == [("P", None), ("Q", None)] and _params(m._jsdiv) == [("P", None), ("Q", None)]
    assert _params(m.jsd_between_point_cloud_sets) == [("sample_pcs", None), ("ref_pcs", None), ("resolution", 28)]


def test_hybrid_trainer_on_cpu_constructs_and_refuses_with_a_reason(tiny_cfg):
    import ldt_amd
    score, comp = ldt_amd.Score(tiny_cfg.score), ldt_amd.Compressor(tiny_cfg.compressor)
    tr = ldt_amd.HybridTrainer(tiny_cfg, score, comp, "cpu")
    assert (tr.epoch, tr.itr, tr.time) == (1, 0, 0.)
    assert isinstance(tr.SDE, ldt_amd.DiffusionVPSDE) and isinstance(tr.optimizer, ldt_amd.EMAWeights)
    assert (tr.N, tr.discrete, tr.time_eps, tr.ode_tol) == (tiny_cfg.sde.train_N, tiny_cfg.opt.discrete, tiny_cfg.sde.time_eps,
                                                            tiny_cfg.sde.ode_tol)
    assert torch.equal(tr.timesteps, torch.linspace(1.0, tiny_cfg.sde.sample_time_eps, tiny_cfg.sde.train_N))
    for sde_type, cls in (("sub_vpsde", ldt_amd.DiffusionSubVPSDE), ("vesde", ldt_amd.DiffusionVESDE)):
        c = copy.deepcopy(tiny_cfg)
        c.sde.sde_type = sde_type
        if sde_type == "vesde":
            c.sde.sigma2_min, c.sde.sigma2_max, c.sde.sigma2_0 = 0.01, 4.0, 0.01
        assert isinstance(ldt_amd.HybridTrainer(c, score, comp, "cpu").SDE, cls)
    c = copy.deepcopy(tiny_cfg)
    c.sde.sde_type = "geometric_sde"
    with pytest.raises(TypeError):                               # Hybrid_Trainer.py:31-32
        ldt_amd.HybridTrainer(c, score, comp, "cpu")
    for call in (lambda: tr.update({}), lambda: tr.update_score(None), lambda: tr.clc_compressor(None), lambda: tr.save()):
        with pytest.raises(NotImplementedError, match="not on this path.*val_nelbo"):
            call()
    with pytest.raises(NotImplementedError, match="mitsuba"):
        tr.valsample([], vis=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):    # no quiet fall-back to eager PyTorch
        tr.val_nelbo({"te_points": torch.zeros(2, 64, 3)})


# ------------------------------------------------------------------------------------------------ JSD helpers
def test_unit_cube_grid_is_the_reference_grid():
    from ldt_amd import metrics as M
    g = golden("jsd")
    res = int(g["resolution"])
    cells, spacing = M.unit_cube_grid_point_cloud(res, True)
    assert cells.dtype == np.float32 and spacing == 1.0 / float(res - 1)
    assert cells.shape == g["grid_sphere"].shape and np.array_equal(cells, g["grid_sphere"])
    cube, _ = M.unit_cube_grid_point_cloud(res)
    assert cube.shape == (res, res, res, 3) and cube.dtype == np.float32
    assert np.array_equal(cube.reshape(-1, 3), g["grid_cube"])
    small, sp = M.unit_cube_grid_point_cloud(3)
    assert sp == 0.5 and np.array_equal(small[2, 0, 1], np.array([0.5, -0.5, 0.0], np.float32))


def test_jensen_shannon_divergence_on_the_stored_counters():
    import warnings
    from ldt_amd import metrics as M
    g = golden("jsd")
    P, Q = g["in/sphere/grid_counters"], g["out/sphere/grid_counters"]
    assert P.dtype == np.float64 and len(P) == len(g["grid_sphere"]) > 10000
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # (the two forms agree: no disagreement warning)
        res = M.jensen_shannon_divergence(P, Q)
    print("JSD %.17g vs the reference's %.17g (difference %.2e)" % (res, float(g["jsd"]), abs(res - float(g["jsd"]))))
    assert abs(res - float(g["jsd"])) <= 1e-12
    assert abs(M._jsdiv(P, Q) - float(g["jsd"])) <= 1e-12
    assert abs(M.jensen_shannon_divergence(Q, Q) - float(g["jsd_self"])) <= 1e-12
    assert abs(M.jensen_shannon_divergence(P * 3.0, Q) - res) <= 1e-12           # normalised inside
    with pytest.raises(ValueError, match="Negative values"):
        M.jensen_shannon_divergence(-P, Q)
    with pytest.raises(ValueError, match="Non equal size"):
        M.jensen_shannon_divergence(P[:-1], Q)
    # the Bernoulli entropy of the reference, from the stored integer counts
    for name in ("in", "out"):
        for tag in ("sphere", "cube"):
            bern = g["%s/%s/bernoulli" % (name, tag)]
            n = float(g["pcs_" + name].shape[0])
            acc = 0.0
            for b in bern[bern > 0]:
                acc += M._entropy([b / n, 1.0 - b / n])
            assert abs(acc / len(bern) - float(g["%s/%s/acc_entropy" % (name, tag)])) <= 1e-12


def test_entropy_of_occupancy_grid_has_no_cpu_path():
    """Host clouds are uploaded where there is a device; where there is none the call raises (no quiet fall-back to a CPU loop)."""
    import contextlib
    from ldt_amd import metrics as M
    g = golden("jsd")
    expect = contextlib.nullcontext() if torch.cuda.is_available() else pytest.raises(RuntimeError, match="no CPU fallback")
    for clouds in (torch.from_numpy(g["pcs_in"][:1]), g["pcs_in"][:1]):
        with expect:
            M.entropy_of_occupancy_grid(clouds, 28, True)


# ------------------------------------------------------------------------------------------------ C-ABI
def test_header_and_binding_agree_on_the_new_entry_points():
    from ldt_amd import _lib
    src = open(os.path.join(ROOT, "include", "ldt_hip.h")).read()
    assert int(re.search(r"#define LDT_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("ldt_nelbo_terms", "ldt_occupancy_grid"):
        m = re.search(r"\bint %s\s*\((.*?)\)\s*;" % name, decl, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name


def test_new_entry_points_return_argument_errors():
    """Null pointers and impossible shapes come back as status codes with a message, before any launch (so no GPU is needed)."""
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib
    lib = _lib.lib()
    assert lib.ldt_nelbo_terms(None, None, None, None, 1, 4, None, None, None) == -1
    assert b"null" in lib.ldt_last_error()
    assert lib.ldt_nelbo_terms(16, 16, 16, None, 1, 4, None, None, None) == -1                 # sample_sums is required
    assert lib.ldt_nelbo_terms(16, 16, None, None, 1, 4, 16, None, None) == -1                 # logqz
    assert lib.ldt_nelbo_terms(16, 16, 16, None, 0, 4, 16, None, None) == -2 and b"nelbo_terms" in lib.ldt_last_error()
    assert lib.ldt_nelbo_terms(16, 16, 16, None, 2, 0, 16, None, None) == -2
    assert lib.ldt_occupancy_grid(None, 1, 1, None, 1, None, None, None) == -1
    assert b"null" in lib.ldt_last_error()
    assert lib.ldt_occupancy_grid(16, 1, 1, 16, 1, 16, None, None) == -1                       # bernoulli
    assert lib.ldt_occupancy_grid(16, 0, 8, 16, 8, 16, 16, None) == -2 and b"occupancy_grid" in lib.ldt_last_error()
    assert lib.ldt_occupancy_grid(16, 1, 0, 16, 8, 16, 16, None) == -2
    assert lib.ldt_occupancy_grid(16, 1, 8, 16, 0, 16, 16, None) == -2
    assert lib.ldt_occupancy_grid(16, 1, 8, 16, 32769, 16, 16, None) == -2                     # more cells than the de-duplication bitmap holds
    with pytest.raises(_lib.LdtHipError, match="no CPU fallback"):
        from ldt_amd import ops
        ops.nelbo_terms(torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(_lib.LdtHipError, match="no CPU fallback"):
        ops.occupancy_grid(torch.zeros(1, 4, 3), torch.zeros(2, 3))
