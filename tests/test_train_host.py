"""CPU: the training surface of `ldt_amd.Trainer` — parameter lists equal to upstream's (trainer/Latent_SDE_Trainer.py:94,111,228), the lazy
`AdamEMA` optimizer and its torch-Adam `state_dict` layout, the refusals (each named, each before any launch), no CPU fallback, and the new
entry points' argument errors (status codes without a launch)."""
import copy
import inspect

import pytest
import torch


def _params(fn, kind=None):
    ps = inspect.signature(fn).parameters.values()
    if kind is inspect.Parameter.KEYWORD_ONLY:
        return [p.name for p in ps if p.kind is kind]
    return [(p.name, None if p.default is inspect.Parameter.empty else p.default) for p in ps
            if p.kind not in (inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.VAR_KEYWORD)]


def _trainer(cfg, cls=None, **score_kw):
    import ldt_amd
    cfg = copy.deepcopy(cfg)
    for k, v in score_kw.items():
        setattr(cfg.score, k, v)
    return (cls or ldt_amd.Trainer)(cfg, ldt_amd.Score(cfg.score), ldt_amd.Compressor(cfg.compressor), "cpu")


def test_signatures_equal_upstream():
    import ldt_amd
    T = ldt_amd.Trainer
    assert _params(T.update) == [("self", None), ("data", None), ("condition", None)]
    assert _params(T.update_score) == [("self", None), ("eps", None), ("condition", None), ("cates", None), ("discrete", False)]
    assert _params(T.update_score, inspect.Parameter.KEYWORD_ONLY) == ["t_index", "eta", "seed"]
    assert _params(T.update, inspect.Parameter.KEYWORD_ONLY) == []
    assert _params(T.save) == [("self", None)] and any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(T.save).parameters.values())
    assert _params(T.warm_up) == [("self", None), ("optimizer", None), ("itr", None)]
    for fn in ("transpose_cast_bf16", "colsum", "wgrad", "dgrad", "layernorm_modulate_bwd", "gelu_bwd", "gate_residual_bwd", "silu_bwd",
               "dsm_loss_bwd", "embedding_grad", "attention_bwd", "sumsq", "adam_ema_step_"):
        assert callable(getattr(ldt_amd.ops, fn)), fn


def test_cpu_trainer_has_a_lazy_adam_ema_optimizer(tiny_cfg):
    import ldt_amd
    tr = _trainer(tiny_cfg)
    opt = tr.optimizer
    assert isinstance(opt, ldt_amd.EMAWeights) and isinstance(opt, ldt_amd.AdamEMA) and isinstance(opt, torch.optim.Optimizer)
    assert len(opt.state) == 0 and opt._flat is None                                  # nothing allocated until the first update
    params = list(tr.model.parameters())
    ref = torch.optim.Adam(params, lr=tiny_cfg.opt.lr, betas=(tiny_cfg.opt.beta1, tiny_cfg.opt.beta2), weight_decay=tiny_cfg.opt.weight_decay)
    torch.optim.lr_scheduler.CosineAnnealingLR(ref, tiny_cfg.common.epochs, 0)       # (adds 'initial_lr', as upstream's scheduler does)
    a, b = opt.state_dict(), ref.state_dict()
    assert a.keys() == b.keys() and a["state"] == {} == b["state"]
    assert len(a["param_groups"]) == 1 and a["param_groups"][0].keys() == b["param_groups"][0].keys()
    assert a["param_groups"][0] == b["param_groups"][0]                               # lr, betas, eps, weight_decay, ..., params 0..n-1
    assert isinstance(tr.scheduler, torch.optim.lr_scheduler.CosineAnnealingLR) and tr.scheduler.T_max == tiny_cfg.common.epochs
    assert opt.param_groups[0]["lr"] == tiny_cfg.opt.lr
    tr.warm_up(opt, 0)
    assert abs(opt.param_groups[0]["lr"] - tiny_cfg.opt.lr / tiny_cfg.opt.warmup_iters) < 1e-15
    opt.swap_parameters_with_ema(store_params_in_ema=True)                            # no EMA yet: a no-op, as upstream
    assert all(p.device.type == "cpu" for p in params) and opt._flat is None


def test_optimizer_state_round_trips_through_load_state_dict(tiny_cfg):
    """A reference-layout state dict (step, moments, ema per parameter) loads on a CPU trainer and comes back out unchanged."""
    tr = _trainer(tiny_cfg)
    params = list(tr.model.parameters())
    g = torch.Generator().manual_seed(0)
    sd = tr.optimizer.state_dict()
    sd["state"] = {i: {"step": torch.tensor(7.0), "exp_avg": torch.randn(p.shape, generator=g), "exp_avg_sq": torch.rand(p.shape, generator=g),
                       "ema": torch.randn(p.shape, generator=g)} for i, p in enumerate(params)}
    tr.optimizer.load_state_dict(sd)
    back = tr.optimizer.state_dict()
    for i, p in enumerate(params):
        assert all(torch.equal(back["state"][i][k], sd["state"][i][k]) for k in ("step", "exp_avg", "exp_avg_sq", "ema"))
        assert torch.equal(tr.optimizer.state[p]["ema"], sd["state"][i]["ema"])
    before = [p.data.clone() for p in params]
    tr.optimizer.swap_parameters_with_ema(store_params_in_ema=True)
    assert all(torch.equal(p.data, sd["state"][i]["ema"]) for i, p in enumerate(params))
    tr.optimizer.swap_parameters_with_ema(store_params_in_ema=True)
    assert all(torch.equal(p.data, b) for p, b in zip(params, before))


def test_update_on_the_cpu_has_no_fallback(tiny_cfg):
    tr = _trainer(tiny_cfg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.update({"tr_points": torch.zeros(2, 64, 3)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.update_score(torch.zeros(2, 8, 120), discrete=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.optimizer.step()
    assert tr.itr == 0 and len(tr.optimizer.state) == 0


def test_refusals_name_their_reason(tiny_cfg, monkeypatch):
    import ldt_amd
    from ldt_amd import dist as ldist
    eps = torch.zeros(2, 8, 120)
    tr = _trainer(tiny_cfg)
    with pytest.raises(NotImplementedError, match="ViPC / point condition"):
        tr.update({"tr_points": torch.zeros(2, 64, 3)}, condition=(torch.zeros(2, 128, 4), 0.))
    with pytest.raises(NotImplementedError, match="ViPC / point condition"):
        tr.update_score(eps, condition={"img": None, "pts": None})
    with pytest.raises(NotImplementedError, match="unet"):
        _trainer(tiny_cfg, unet=True).update_score(eps)
    with pytest.raises(NotImplementedError, match="norm='group_norm'.*layer_norm"):
        _trainer(tiny_cfg, norm="group_norm").update_score(eps)
    with pytest.raises(NotImplementedError, match="dropout=0.1"):
        _trainer(tiny_cfg, dropout=0.1).update_score(eps)
    monkeypatch.setattr(ldist, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="2 ranks.*all-reduce"):
        tr.update_score(eps)
    monkeypatch.undo()
    with pytest.raises(NotImplementedError, match="ViPC / point condition"):
        _trainer(tiny_cfg, cls=ldt_amd.CompletionTrainer).update({"tr_points": torch.zeros(2, 64, 3)})
    assert tr.itr == 0 and tr.optimizer._flat is None                                 # refused before anything was launched or allocated


def test_untrained_trainers_keep_refusing(tiny_cfg):
    import ldt_amd
    hy = _trainer(tiny_cfg, cls=ldt_amd.HybridTrainer)
    for call in (lambda: hy.update({}), lambda: hy.update_score(None), lambda: hy.clc_compressor(None), lambda: hy.save()):
        with pytest.raises(NotImplementedError):
            call()
    ct = ldt_amd.CompressorTrainer(tiny_cfg, ldt_amd.Compressor(tiny_cfg.compressor), "cpu")
    with pytest.raises(NotImplementedError, match="not on this path"):
        ct.update({})


def test_new_entry_points_return_argument_errors():
    """Null pointers and impossible shapes come back as status codes with a message (no launch, so no GPU needed)."""
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib
    lib = _lib.lib()
    assert lib.ldt_abi_version() == 26
    assert lib.ldt_transpose_cast_bf16(None, 0, 8, None, 64, 8, 8, 64, None) == -1
    assert lib.ldt_transpose_cast_bf16(16, 0, 8, 16, 32, 8, 8, 64, None) == -2           # ld_dst < R_pad
    assert lib.ldt_colsum(None, 0, 8, 8, 8, None, None) == -1 and lib.ldt_colsum(16, 0, 4, 8, 8, 16, None) == -2
    assert lib.ldt_layernorm_modulate_bwd(16, 8, 16, 8, None, 0, 3, 16, 8, None, None, 0, 16, 8, 8, None) == -2    # 8 rows, samples of 3
    assert lib.ldt_layernorm_modulate_bwd(16, 8, 16, 8, None, 0, 4, 16, 8, 16, None, 8, 16, 8, 8, None) == -1      # dshift without dscale
    assert lib.ldt_gelu_bwd(None, 8, 16, 0, 8, 16, 8, 8, 8, None) == -1
    assert lib.ldt_gate_residual_bwd(16, 8, None, 0, 0, 16, 0, 4, 16, 8, 16, 8, 8, 8, None) == -1 and b"dgate" in lib.ldt_last_error()
    assert lib.ldt_silu_bwd(16, None, 16, None, 8, None) == -1
    assert lib.ldt_dsm_loss_bwd(16, 16, None, 0, 8, 0, 16, None) == -2
    assert lib.ldt_embedding_grad(16, 4, 16, 2, 8, 3, 16, None) == -2                   # ld < D
    args = [16, 128, 1024, 16, 128, 16, 128, 1024, 16, 16, 16, 16, 128, 1024, 16, 128, 16, 128, 1024]
    assert lib.ldt_attention_bwd(*args, 1, 2, 8, 32, None) == -2 and b"64 only" in lib.ldt_last_error()
    assert lib.ldt_attention_bwd(*args, 1, 2, 513, 64, None) == -2
    assert lib.ldt_attention_bwd(*(args[:1] + [132] + args[2:]), 1, 2, 8, 64, None) == -3   # rows not 16-byte aligned
    assert lib.ldt_sumsq(16, 0, 16, 8, 0., 16, None) == -2
    assert lib.ldt_adam_ema_step(16, 16, 16, 16, None, 8, 1e-3, .9, .999, 1e-8, 0., 0, 0., 0, None, None) == -2 and b"from 1" in lib.ldt_last_error()
