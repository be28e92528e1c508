"""GPU (-m gpu): whole Score training steps at head widths 8, 16 and 32 against tests/golden/score_train_narrow.npz
(tools/gen_score_train_narrow_golden.py: the reference's own `Trainer.update_score` on the CPU and a bf16 twin's distance from it), with the
bars of test_gpu_train.py — stated with their reason at the top of that file.  Helpers: tests/train_narrow_checks.py.

    (a) 16 heads x 8, T = 32 (the hybrid config's Score layout): iteration 0 and the 20-step trajectory, update and optimizer state
    (b) 8 heads x 16, T = 40, three classes with labels: iteration 0
    (c) 4 heads x 32, T = 24: iteration 0
and two `Trainer.update` calls on a config that carries the hybrid YAML's score section at 2 blocks.  Measured values are printed (-s) and
recorded in DESIGN.md section 4.13.  Before the narrow attention backward existed every test here ended at refuse_untrainable."""
import copy

import numpy as np
import pytest
import torch

import train_narrow_checks as tn
from train_narrow_checks import rel_mse

pytestmark = pytest.mark.gpu


def make_trainer(cfg, key):
    import ldt_amd
    score, init = tn.initial_score(cfg, key)
    comp = ldt_amd.Compressor(cfg.compressor)
    comp.init()
    return ldt_amd.Trainer(cfg, score, comp, "cuda"), init


@pytest.mark.parametrize("key", list(tn.MODELS))
def test_iteration0_gradients_and_loss(tiny_cfg, key):
    g = tn.golden()
    ref, names, _ = tn.reference_grads0(tiny_cfg, key)
    tr, _ = make_trainer(tn.train_cfg(tiny_cfg, key, grad_norm_clip_value=None), key)   # no clipping: p.grad stays the raw gradient
    idx, eta = tn.draw(key, 0)
    cates = tn.cates_of(key)
    loss = tr.update_score(tn.eps_of(key).cuda(), cates=None if cates is None else cates.cuda(), discrete=True, t_index=idx, eta=eta)
    assert loss.shape == () and loss.is_cuda
    want = float(g[key + "_loss"][0])
    print("(%s) train loss, iteration 0: %.7f vs the reference's %.7f (relative %.2e)" % (key, float(loss), want, abs(float(loss) - want) / want))
    assert abs(float(loss) - want) <= 1e-3 * want
    named = dict(tr.model.named_parameters())
    assert list(named) == names
    allb = float(g[key + "_twin_grad_relmse_all"])
    worst = 0.0
    for n in names:
        got = named[n].grad
        assert got is not None and got.shape == ref[n].shape and bool(torch.isfinite(got).all()), n
        e, bar = rel_mse(got.cpu(), ref[n]), 2 * max(float(g[key + "_twin_grad_relmse::" + n]), allb)
        worst = max(worst, e / bar)
        assert e <= bar, "%s: gradient rel-MSE %.3e > %.3e (2 x the bf16 twin's)" % (n, e, bar)
    e_all = rel_mse(torch.cat([named[n].grad.reshape(-1) for n in names]).cpu(), torch.cat([ref[n].reshape(-1) for n in names]))
    print("(%s) gradient rel-MSE, all parameters: %.3e = %.2f x the twin's %.3e; worst per-tensor ratio to its bar %.2f" % (key, e_all, e_all / allb, allb, worst))
    assert e_all <= 2 * allb


def test_hybrid_layout_loss_trajectory_and_optimizer_state(tiny_cfg):
    g = tn.golden()
    tr, init = make_trainer(tn.train_cfg(tiny_cfg, "a"), "a")
    eps = tn.eps_of("a").cuda()
    losses = []
    for i in range(20):
        idx, eta = tn.draw("a", i)
        tr.itr = i                                                                # the fixture drives update_score directly: warm-up by itr
        losses.append(float(tr.update_score(eps, discrete=True, t_index=idx, eta=eta)))
        if i == 0:                                                                # after iteration 1: every entry exists, reference shapes
            params = list(tr.model.parameters())
            shapes = [str(s) for s in g["a_opt_shapes"]]
            assert len(tr.optimizer.state) == len(params) == len(shapes)
            for p, want in zip(params, shapes):
                st = tr.optimizer.state[p]
                assert sorted(st) == [str(k) for k in g["a_opt_keys"]]
                assert ";".join("x".join(map(str, v.shape)) for v in (p, st["exp_avg"], st["exp_avg_sq"], st["ema"])) == want
                assert float(st["step"]) == float(g["a_opt1_step"]) == 1.0
    ref = g["a_loss"].tolist()
    dev = max(abs(a - b) / b for a, b in zip(losses, ref))
    twin = float(g["a_twin_loss_dev"])
    print("(a) 20-step loss trajectory: %.4f -> %.4f (reference %.4f -> %.4f); worst relative deviation %.3e = %.2f x the twin's %.3e"
          % (losses[0], losses[-1], ref[0], ref[-1], dev, dev / twin, twin))
    assert losses[-1] < 0.7 * losses[0]                                           # it trains
    assert dev <= 2 * twin
    assert abs(tr.optimizer.param_groups[0]["lr"] - 2e-3) < 1e-12 and float(tr.optimizer.state[params[0]]["step"]) == 20.0
    named = dict(tr.model.named_parameters())
    small = [n for n in named if "a_after20::" + n in g]
    assert len(small) == 17                                                       # every bias of the unconditional two-block Score
    upd = lambda vals, key: (torch.cat([(v.cpu() - init[n]).reshape(-1) for n, v in zip(small, vals)]),
                             torch.cat([(g[key + n] - init[n]).reshape(-1) for n in small]))
    e_w = rel_mse(*upd([named[n].data for n in small], "a_after20::"))
    e_e = rel_mse(*upd([tr.optimizer.state[named[n]]["ema"] for n in small], "a_ema20::"))
    print("(a) 20-step update of the small tensors: weights rel-MSE %.3e = %.2f x the twin's, EMA %.3e = %.2f x the twin's"
          % (e_w, e_w / float(g["a_twin_after20_update_relmse"]), e_e, e_e / float(g["a_twin_ema20_update_relmse"])))
    assert e_w <= 2 * float(g["a_twin_after20_update_relmse"]) and e_e <= 2 * float(g["a_twin_ema20_update_relmse"])


def test_update_on_the_hybrid_score_section(tiny_cfg):
    """`Trainer.update` (encode with a frozen small Compressor, then update_score) on a config whose score section is the hybrid YAML's
    (hidden 128, 16 heads, t_dim 128, z 120, 32 tokens) at 2 blocks."""
    import ldt_amd
    cfg = copy.deepcopy(tiny_cfg)
    cfg.score.hidden_size, cfg.score.num_heads, cfg.score.t_dim, cfg.score.z_dim, cfg.score.z_scale, cfg.score.num_blocks = 128, 16, 128, 120, 32, 2
    cfg.compressor.z_scales = 32
    assert cfg.compressor.z_dim * cfg.compressor.n_layers == cfg.score.z_dim and cfg.data.tr_max_sample_points == 64
    torch.manual_seed(3)
    comp = ldt_amd.Compressor(cfg.compressor)
    comp.init()
    tr = ldt_amd.Trainer(cfg, ldt_amd.Score(cfg.score), comp, "cuda")
    g = torch.Generator().manual_seed(3)
    pts = torch.randn(4, 64, 3, generator=g)
    pts = pts - pts.mean(1, keepdim=True)
    data = {"tr_points": pts / pts.norm(dim=-1).amax(1)[:, None, None]}
    np.random.seed(5); torch.manual_seed(5)
    for i in range(2):
        loss = tr.update(data)
        assert loss.shape == () and bool(torch.isfinite(loss)) and tr.itr == i + 1
    assert tr.itr == 2
