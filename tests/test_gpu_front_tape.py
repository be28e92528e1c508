"""GPU (-m gpu): one FrontTrainStep forward + backward audited call by call (tests/front_tape.py), at the tiny shape (hidden 64, 8 tokens of
16 neighbours, N = 64, B = 3) with the parameters' `.grad` as views of an optimizer's flat buffer, and at a ragged one (hidden 128, 24 tokens
of 8 neighbours, N = 96, B = 2, norm_input on).  Every call of the six new entry points, of the GEMMs, the column sums and the fp32 linears
is held per element against its float64 reference on the operands the step handed it; the number of calls of each kind is the step's.

Before the step existed the test ended at the missing `FrontTrainStep`."""
import copy

import pytest
import torch

import front_tape as ft

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", ["tiny", "ragged"])
def test_front_step_call_by_call(tiny_cfg, shape, monkeypatch):
    import ldt_amd
    from ldt_amd import compressor_train as ct
    c = copy.deepcopy(tiny_cfg.compressor)
    B = 3
    if shape == "ragged":
        c.hidden_dim, c.num_heads, c.p_dim, c.z_scales, c.outsize, c.max_outputs, c.norm_input = 128, 4, 40, 24, 96, 96, True
        B = 2
    torch.manual_seed(4)
    model = ldt_amd.Compressor(c).cuda().train()
    if shape == "tiny":                                                 # .grad views of a flat buffer, 4-byte aligned, as update_front hands them
        opt = ldt_amd.AdamEMA([p for _, p in ct.front_parameters(model)], lr=1e-3, ema_decay=0.)
        opt.zero_grad()
    g = torch.Generator().manual_seed(9)
    cloud = torch.randn(B, c.outsize, 3, generator=g) * 0.5
    d_tok = torch.randn(B, c.z_scales, c.hidden_dim, generator=g) * 0.1
    d_pos = torch.randn(B, c.p_dim, generator=g) * 0.1
    rec = ft.Recorder(ct.ops)
    monkeypatch.setattr(ct, "ops", rec)
    step = ct.FrontTrainStep(model)
    step.forward(cloud.cuda())
    step.backward(d_tok.cuda(), d_pos.cuda())
    monkeypatch.undo()
    worst = ft.audit(rec.calls)
    print("front tape %s: " % shape + "  ".join("%s x%d %.3f" % (k, v[0], v[1]) for k, v in sorted(worst.items())))
    assert {k: v[0] for k, v in worst.items()} == ft.EXPECTED
    assert all(p.grad is not None and bool(p.grad.isfinite().all()) for _, p in ct.front_parameters(model))
