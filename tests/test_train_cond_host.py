"""Host checks (no GPU) for Score training on a ViPC condition pair: the cross-attention backward's reference and bound
(kernel_checks.attn_bwd_ref at two lengths, on the cases of tests/cross_bwd_checks.py), an fp32 emulation of the kernels with planted faults,
the argument checks of ldt_attention_bwd_cross, the refusals of `CompletionTrainer`, and the fixture tests/golden/score_train_cond.npz
against the oracle (tests/train_cond_checks.py)."""
import copy
import inspect

import pytest
import torch

import cross_bwd_checks as cb
import narrow_bwd_checks as nb
import train_cond_checks as tc


# ------------------------------------------------------------------------------------------------ the reference and its bound
@pytest.mark.parametrize("B,H,Nq,Nk,Dh,large", cb.CASES)
def test_emulation_is_inside_the_bound(B, H, Nq, Nk, Dh, large):
    """fp32 products, fp32 L and D, bf16 outputs: inside the bound in the form the kernel of that width takes, at every shape the GPU test runs."""
    q, kv, do = cb.cross_case(B, H, Nq, Nk, Dh, large)
    o = nb.forward_o(q, kv, B, H, Nq, Nk, Dh)
    r = nb.check(nb.emulate(q, kv, o, do, B, H, Nq, Nk, Dh, nb.rounds(Dh)), q, kv, o, do, B, H, Nq, Nk, Dh, "emulation")
    print("emulation B%d H%d Nq%d Nk%d Dh%d large=%d: err / tol %.3f" % (B, H, Nq, Nk, Dh, large, r))
    assert r <= 1.0
    if large:
        s = nb.scores64(q, kv, B, H, Nq, Nk, Dh)
        assert float(s.amax(-1).min()) > 25 and float(s.amax(-1).max()) > 89


@pytest.mark.parametrize("fault,B,H,Nq,Nk,Dh,output", [
    ("last key dropped from dq", 2, 2, 8, 24, 64, "dq"),
    ("last key dropped from dq", 1, 2, 17, 33, 8, "dq"),
    ("last query dropped from dk dv", 1, 2, 72, 40, 64, "d[kv]"),
    ("last query dropped from dk dv", 2, 3, 33, 17, 16, "d[kv]"),
    ("stats of Nk rows", 2, 2, 8, 24, 64, "d[qkv]"),
    ("stats of Nk rows", 2, 4, 17, 33, 32, "d[qkv]"),
    ("D not subtracted", 2, 3, 33, 17, 16, "d[qk]"),
])
def test_planted_faults_fail_naming_the_output(fault, B, H, Nq, Nk, Dh, output):
    q, kv, do = cb.cross_case(B, H, Nq, Nk, Dh)
    o = nb.forward_o(q, kv, B, H, Nq, Nk, Dh)
    with pytest.raises(AssertionError, match=r"planted %s: \d+ of \d+ elements outside the bound" % output):
        nb.check(nb.emulate(q, kv, o, do, B, H, Nq, Nk, Dh, nb.rounds(Dh), fault=fault), q, kv, o, do, B, H, Nq, Nk, Dh, "planted")


@pytest.mark.parametrize("B,H,Nq,Nk,Dh", cb.PROBES)
def test_selection_probe_is_exact_in_the_emulation(B, H, Nq, Nk, Dh):
    q, kv, do, pi, lead = cb.selection_probe(B, H, Nq, Nk, Dh, seed=31 + Nq + Nk + Dh)
    s = nb.scores64(q, kv, B, H, Nq, Nk, Dh)
    top2 = s.topk(2, -1).values
    assert lead >= 110 and torch.equal(s.argmax(-1), pi) and float((top2[..., 0] - top2[..., 1]).min()) >= 110
    assert all(len(set(row.tolist())) == Nq for row in pi.reshape(-1, Nq))            # every key wins at most one query
    o = nb.forward_o(q, kv, B, H, Nq, Nk, Dh)
    want = cb.selection_expected_dv(do, pi, B, H, Nq, Nk, Dh)
    for rounded in (True, False):
        assert torch.equal(nb.emulate(q, kv, o, do, B, H, Nq, Nk, Dh, rounded)["dv"], want)
    moved = nb.emulate(q, kv, o, do, B, H, Nq, Nk, Dh, True, fault="last query dropped from dk dv")["dv"]
    assert not torch.equal(moved, want)


# ------------------------------------------------------------------------------------------------ the entry point and its surface
def test_cross_entry_point_returns_argument_errors():
    """Null pointers, head widths, lengths, strides and alignment come back as status codes with a message: no launch, so no GPU needed."""
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib, ops
    lib = _lib.lib()
    assert lib.ldt_abi_version() == 26 == _lib.ABI_VERSION
    assert "ldt_attention_bwd_cross" in _lib.SIGNATURES and len(_lib.SIGNATURES["ldt_attention_bwd_cross"]) == len(_lib.SIGNATURES["ldt_attention_bwd"]) + 1
    assert callable(ops.attention_bwd_cross)
    assert list(inspect.signature(ops.attention_bwd_cross).parameters) == ["q", "k", "v", "o", "do", "B", "H", "Nq", "Nk", "head_dim", "dq_out", "dkv_out"]
    args = [16, 128, 1024, 16, 128, 16, 128, 1024, 16, 16, 16, 16, 128, 1024, 16, 128, 16, 128, 1024]
    f = lib.ldt_attention_bwd_cross
    assert f(*([None] + args[1:]), 1, 2, 8, 8, 8, None) == -1 and b"null" in lib.ldt_last_error()
    assert f(*(args[:10] + [None] + args[11:]), 1, 2, 8, 8, 8, None) == -1          # stats
    for dh in (24, 128, 0):
        assert f(*args, 1, 2, 8, 8, dh, None) == -2 and b"8, 16, 32 or 64" in lib.ldt_last_error()
    for dh in (8, 16, 32, 64):
        assert f(*args, 1, 2, 513, 8, dh, None) == -2 and b"Nq 513" in lib.ldt_last_error()
        assert f(*args, 1, 2, 8, 513, dh, None) == -2 and b"Nk 513" in lib.ldt_last_error()
        assert f(*args, 1, 2, 0, 8, dh, None) == -2 and f(*args, 1, 2, 8, 0, dh, None) == -2 and f(*args, 0, 2, 8, 8, dh, None) == -2
        assert f(*(args[:1] + [132] + args[2:]), 1, 2, 8, 8, dh, None) == -3        # Q rows not 16-byte aligned
        assert f(*(args[:4] + [132] + args[5:]), 1, 2, 8, 8, dh, None) == -3        # K rows
    assert f(*(args[:1] + [24] + args[2:]), 1, 4, 8, 8, 8, None) == -2 and b"shorter than heads" in lib.ldt_last_error()   # 24 < 4 x 8
    assert f(*(args[:12] + [130] + args[13:]), 1, 2, 8, 8, 8, None) == -3 and b"8-byte aligned" in lib.ldt_last_error()    # dQ rows, narrow heads
    assert f(*(args[:15] + [130] + args[16:]), 1, 2, 8, 8, 16, None) == -3          # dK rows, narrow heads


def _trainer(cfg, cls, **score_kw):
    import ldt_amd
    cfg = copy.deepcopy(cfg)
    for k, v in score_kw.items():
        setattr(cfg.score, k, v)
    return cls(cfg, ldt_amd.Score(cfg.score), ldt_amd.Compressor(cfg.compressor), "cpu")


def test_completion_trainer_signatures_follow_upstream():
    import ldt_amd
    T = ldt_amd.CompletionTrainer
    pos = lambda fn: [(p.name, None if p.default is inspect.Parameter.empty else p.default) for p in inspect.signature(fn).parameters.values()
                      if p.kind is not inspect.Parameter.KEYWORD_ONLY]
    assert pos(T.update) == [("self", None), ("data", None), ("condition", None)]
    assert pos(T.update_score) == [("self", None), ("eps", None), ("condition", None), ("cates", None), ("discrete", True)]
    assert [p.name for p in inspect.signature(T.update_score).parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY] == ["t_index", "eta", "seed"]


def test_completion_trainer_refusals_name_their_reason(tiny_cfg, monkeypatch):
    import ldt_amd
    from ldt_amd import dist as ldist
    from ldt_amd.train import refuse_untrainable
    eps, data = torch.zeros(2, 8, 120), torch.zeros(2, 64, 3)
    pair = (torch.zeros(2, 128, 4), torch.zeros(2, 128))
    ct = _trainer(tiny_cfg, ldt_amd.CompletionTrainer)
    for call in (lambda: ct.update(data), lambda: ct.update({"tr_points": data}), lambda: ct.update_score(eps)):
        with pytest.raises(NotImplementedError, match=r"ViPC / point condition.*\(pts_condition, img_condition\) pair.*unconditional step is Trainer\.update"):
            call()
    raw = {"img": torch.zeros(2, 3, 3, 8, 8), "pts": torch.zeros(2, 16, 3)}
    for call in (lambda: ct.update(data, condition=raw), lambda: ct.update_score(eps, condition=raw)):
        with pytest.raises(NotImplementedError, match=r"ConditionNet's backward is missing.*model\.c_net\(condition\).*freezes ConditionNet"):
            call()
    with pytest.raises(TypeError, match="pair"):
        ct.update_score(eps, condition=torch.zeros(2, 128, 4))
    # every other refusal of refuse_untrainable applies unchanged
    with pytest.raises(NotImplementedError, match="unet"):
        _trainer(tiny_cfg, ldt_amd.CompletionTrainer, unet=True).update_score(eps, condition=pair)
    with pytest.raises(NotImplementedError, match="norm='group_norm'.*layer_norm"):
        _trainer(tiny_cfg, ldt_amd.CompletionTrainer, norm="group_norm").update_score(eps, condition=pair)
    with pytest.raises(NotImplementedError, match="dropout=0.1"):
        _trainer(tiny_cfg, ldt_amd.CompletionTrainer, dropout=0.1).update_score(eps, condition=pair)
    monkeypatch.setattr(ldist, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="2 ranks.*all-reduce"):
        ct.update_score(eps, condition=pair)
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="no CPU fallback"):                          # a pair on a CPU trainer: past the refusals
        ct.update_score(eps, condition=pair)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ct.update(data, condition=pair)
    assert ct.itr == 0 and ct.optimizer._flat is None and ct.last_condition_grad is None
    # a ConditionNet in the model: its parameters would receive a zero gradient, which weight decay turns into a silent decay
    cfg = copy.deepcopy(tiny_cfg)
    cfg.opt.weight_decay = 0.01
    cn = _trainer(cfg, ldt_amd.CompletionTrainer, condition=True)
    assert hasattr(cn.model, "c_net")
    for call in (lambda: cn.update(data, condition=pair), lambda: cn.update_score(eps, condition=pair)):
        with pytest.raises(NotImplementedError, match=r"weight_decay=0.01 with a ConditionNet.*zero gradient.*silently decay"):
            call()
    assert cn.itr == 0 and cn.optimizer._flat is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):                          # without weight decay the same model passes the refusals
        _trainer(tiny_cfg, ldt_amd.CompletionTrainer, condition=True).update_score(eps, condition=pair)
    # the base Trainer keeps refusing every condition; refuse_untrainable's default is to refuse
    tr = _trainer(tiny_cfg, ldt_amd.Trainer)
    with pytest.raises(NotImplementedError, match="ViPC / point condition"):
        tr.update({"tr_points": data}, condition=pair)
    with pytest.raises(NotImplementedError, match="ViPC / point condition"):
        tr.update_score(eps, condition=pair)
    with pytest.raises(NotImplementedError, match="self-attention blocks only"):
        refuse_untrainable(tr.model, pair)
    refuse_untrainable(tr.model, pair, allow_condition=True)
    with pytest.raises(NotImplementedError, match="self-attention blocks only"):
        ldt_amd.train.ScoreTrainStep(cn.model)
    assert tr.itr == 0 and tr.optimizer._flat is None


# ------------------------------------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("key", list(tc.MODELS))
def test_fixture_is_tied_to_the_oracle(tiny_cfg, key):
    """The initial weights, latents and conditions rebuilt from their seeds match the stored digests, and the fp32 oracle's iteration-0
    gradients — with respect to the parameters AND to the condition pair — and loss match grad0_digest::* / dcond_* / loss[0] (all asserted
    inside reference_grads0, at the bars test_train_narrow_host.py uses for score_train_narrow), as test_gpu_train_cond.py relies on."""
    g = tc.golden()
    grads, names, d_pts, d_img, loss = tc.reference_grads0(tiny_cfg, key)
    m = tc.MODELS[key]
    assert len(names) == len(grads) and g[key + "_idx"].shape == (m["iters"], m["B"]) and g[key + "_loss"].shape == (m["iters"],)
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())
    assert float(g[key + "_twin_grad_relmse_all"]) > 0 and all(key + "_twin_grad_relmse::" + n in g for n in names)
    assert tuple(d_pts.shape) == (m["B"], tc.HIDDEN, m["S"]) and float(d_pts.abs().max()) > 0 and float(g[key + "_twin_dcond_relmse::pts"]) > 0
    cross = [n for n in names if ".fc_kv." in n]
    assert len(cross) == 2 * m["num_blocks"] and all(float(grads[n].abs().max()) > 0 for n in cross)
    if key == "z":
        assert d_img is None and torch.equal(g["z_cates"], tc.CATES["z"]) and "z_twin_dcond_relmse::img" not in g
    else:
        assert tuple(d_img.shape) == (m["B"], tc.T_DIM) and float(d_img.abs().max()) > 0 and float(g[key + "_twin_dcond_relmse::img"]) > 0
    if key == "x":
        assert float(g["x_loss"][-1]) < 0.7 * float(g["x_loss"][0]) and float(g["x_twin_loss_dev"]) > 0
