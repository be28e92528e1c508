"""CPU (no GPU needed): the front training step's host side (ldt_amd/compressor_train.py: FrontTrainStep, front_parameters,
refuse_untrainable_front; CompressorTrainer.update_front), the new entry points (csrc/batchnorm.hip, csrc/grouper_bwd.hip) and the helpers
of tests/front_train_checks.py.

  * the six entry points are in the header, in the binding's table and in the built library; the ABI stays 26; their argument errors come
    back as status codes with a message: no launch
  * front_parameters + encoder_parameters + topdown_parameters is named_parameters exactly, on the tiny and on the shipped shape
  * every refusal of refuse_untrainable_front fires with its reason; update_front is keyword-only behind `data`, refuses on a CPU device
    with nothing allocated, the completion trainer refuses, update / compute_loss keep their messages
  * the float64 references of the four new kernels equal torch autograd (BatchNorm1d in training mode + ReLU; max over ReLU; the 'anchor'
    grouping), and the running buffers equal nn.BatchNorm1d's
  * the fp32 emulation of the BatchNorm kernels sits inside the bounds on every case, and each planted fault leaves them by more than 3 x on
    some case: biased / unbiased variance swapped in rstd and in running_var, the xhat dgamma / M term dropped, the mask taken from dy, fp32
    running sums at M = 70 000; for the grouping: the anchor's -sum_j dd dropped, the P term dropped; for the max: the last equal index
  * the restated front with its own selections is torch autograd through relu / max; pinned to another run's selections it differentiates
    at those

Which of these depend on the feature: the entry-point tests (declared / bound / built, status codes), the parameter-list union, the refusals
and the `update_front` signature test end at a missing symbol or attribute without it.  The others (the references against torch autograd,
the emulation and the planted faults, the restated front) hold the helpers of tests/front_train_checks.py alone, which the GPU tests stand
on: they pass with or without the step."""
import copy
import inspect
import re

import pytest
import torch

import front_train_checks as fc
import kernel_checks as kc
from conftest import rel_mse

ENTRIES = ("ldt_bn_stats", "ldt_bn_relu_fwd", "ldt_bn_relu_bwd", "ldt_maxpool_argmax", "ldt_maxpool_relu_bwd", "ldt_group_normalize_bwd")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib
    return _lib


def _compressor(tiny_cfg, **kw):
    import ldt_amd
    c = copy.deepcopy(tiny_cfg.compressor)
    for k, v in kw.items():
        setattr(c, k, v)
    return ldt_amd.Compressor(c)


def test_entry_points_are_declared_bound_and_built(built):
    src = open(built._HERE + "/../include/ldt_hip.h").read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, decl) and name in built.SIGNATURES and hasattr(built.lib(), name), name
        n_args = len(re.search(r"\bint %s\s*\(([^)]*)\)" % name, decl).group(1).split(","))
        assert len(built.SIGNATURES[name]) == n_args, name
    assert built.ABI_VERSION == 26 and built.lib().ldt_abi_version() == 26


def test_entry_points_return_status_codes_before_any_launch(built):
    L, err = built.lib(), built.lib().ldt_last_error
    assert L.ldt_bn_stats(None, 8, 4, 8, 1e-5, 16, None, None, 0.1, None) == -1 and b"bn_stats: null pointer" in err()
    assert L.ldt_bn_stats(16, 8, 1, 8, 1e-5, 16, None, None, 0.1, None) == -2 and b"more than one value per channel" in err()
    assert L.ldt_bn_relu_fwd(16, 8, 4, 8, 16, 16, 16, None, 8, 1, 8, None) == -1 and b"bn_relu_fwd: null pointer" in err()
    assert L.ldt_bn_relu_fwd(16, 8, 4, 8, 16, 16, 16, 16, 8, 1, 64, None) == -2
    assert L.ldt_bn_relu_bwd(16, 8, 16, 8, 4, 8, None, 16, 16, 16, 8, None, None, None) == -1 and b"bn_relu_bwd: null pointer" in err()
    assert L.ldt_bn_relu_bwd(16, 8, 16, 8, 1, 8, 16, 16, 16, 16, 8, None, None, None) == -2
    assert L.ldt_maxpool_argmax(16, 0, 8, 2, 4, 8, 16, None, 0, None) == -1 and L.ldt_maxpool_argmax(16, 0, 8, 0, 4, 8, 16, 16, 0, None) == -2
    assert L.ldt_maxpool_relu_bwd(16, None, 16, 2, 4, 8, 16, 8, None) == -1 and L.ldt_maxpool_relu_bwd(16, 16, 16, 2, 4, 8, 16, 7, None) == -2
    g = [16, 0, 19, 16, 16, 16, 16, 16, 16, 16, 2, 8, 2, 4, 8, 16, 16, 16, None]
    for i in (0, 3, 4, 5, 6, 9):
        a = list(g)
        a[i] = None
        assert L.ldt_group_normalize_bwd(*a) == -1 and b"group_normalize_bwd: null pointer" in err(), i
    a = list(g)
    a[7] = None
    assert L.ldt_group_normalize_bwd(*a) == -1 and b"inverted index" in err()
    a = list(g)
    a[2] = 18                                                            # ld < 2 D + 3
    assert L.ldt_group_normalize_bwd(*a) == -2
    from ldt_amd import ops
    with pytest.raises(built.LdtHipError, match="x must be a device tensor.*no CPU fallback"):
        ops.bn_stats(torch.zeros(4, 8))
    with pytest.raises(built.LdtHipError, match="no CPU fallback"):
        ops.maxpool_argmax(torch.zeros(8, 8), 2, 4)


@pytest.mark.parametrize("shape", ["tiny", "shipped"])
def test_the_three_parameter_lists_cover_the_compressor(tiny_cfg, shape):
    from ldt_amd.compressor_train import encoder_parameters, front_parameters, topdown_parameters
    kw = {} if shape == "tiny" else dict(hidden_dim=128, num_heads=4, n_layers=6, encoder_layers=2, p_dim=256, z_scales=32, z_dim=20)
    m = _compressor(tiny_cfg, **kw)
    fr, en, top = ([n for n, _ in f(m)] for f in (front_parameters, encoder_parameters, topdown_parameters))
    every = [n for n, _ in m.named_parameters()]
    assert len(fr) + len(en) + len(top) == len(every) and set(fr) | set(en) | set(top) == set(every)
    assert fr == [n for n in every if n in set(fr)]                      # module order
    ex = "group.extraction."
    assert fr == ["input.weight", "input.bias", "group.affine_alpha", "group.affine_beta"] + [ex + n + s for n in (
        "transfer.net.0", "transfer.net.1", "operation.0.net1.0", "operation.0.net1.1", "operation.0.net2.0") for s in (".weight", ".bias")] + [
        "pos_embedding." + n + s for n in ("conv1", "conv2", "bn1", "bn2", "fc") for s in (".weight", ".bias")]
    assert all(p is dict(m.named_parameters())[n] for n, p in front_parameters(m))
    assert fr == fc.front_names(m.state_dict())


def test_refuse_untrainable_front_names_each_reason(tiny_cfg):
    from ldt_amd.compressor_train import FrontTrainStep, refuse_untrainable_front
    for kw, msg in ((dict(pre_group=True), "pre_group: True.*two chained groupers"),
                    (dict(pos_embedding="mlp"), "pos_embedding: mlp.*MiniPointnet"),
                    (dict(class_condition=True, num_categorys=3), "class_condition"),
                    (dict(cluster_norm="center"), "cluster_norm='center'.*'anchor' only")):
        with pytest.raises(NotImplementedError, match=msg):
            FrontTrainStep(_compressor(tiny_cfg, **kw))
    m = _compressor(tiny_cfg)
    with pytest.raises(NotImplementedError, match="7 points in 8 groups.*k = N // T \\* 2 = 0"):
        refuse_untrainable_front(m, num_points=7)
    with pytest.raises(RuntimeError, match="parameters are on cpu.*no CPU fallback"):   # the last refusal: everything else works on CPU parameters
        refuse_untrainable_front(m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FrontTrainStep(m)
    assert list(inspect.signature(FrontTrainStep.forward).parameters) == ["self", "x"]
    assert list(inspect.signature(FrontTrainStep.backward).parameters) == ["self", "d_tokens", "d_pos"]
    assert list(inspect.signature(refuse_untrainable_front).parameters) == ["model", "num_points"]


def test_update_front_signature_and_refusals(tiny_cfg):
    import ldt_amd
    sig = inspect.signature(ldt_amd.CompressorTrainer.update_front)
    assert list(sig.parameters) == ["self", "data", "post_noise"]
    assert [p.name for p in sig.parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY] == ["post_noise"]
    tr = ldt_amd.CompressorTrainer(tiny_cfg, ldt_amd.Compressor(tiny_cfg.compressor), "cpu")
    assert tr.front_optimizer is None
    with pytest.raises(ValueError, match="update_front: cfg.opt.kl_weight is not set"):
        tr.update_front({"tr_points": torch.zeros(2, 64, 3)})
    cfg = copy.deepcopy(tiny_cfg)
    cfg.opt.kl_weight = 0.5
    tr = ldt_amd.CompressorTrainer(cfg, ldt_amd.Compressor(cfg.compressor), "cpu")
    before = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.update_front({"tr_points": torch.zeros(2, 64, 3)})
    assert tr.front_optimizer is None and tr.encoder_optimizer is None and tr.itr == 0 and all(p.grad is None for p in tr.model.parameters())
    assert all(torch.equal(v, before[k]) for k, v in tr.model.state_dict().items())          # the running buffers too
    for kw, msg in ((dict(pre_group=True), "pre_group: True"), (dict(pos_embedding="mlp"), "pos_embedding: mlp")):
        bad = ldt_amd.CompressorTrainer(cfg, _compressor(cfg, **kw), "cpu")
        with pytest.raises(NotImplementedError, match=msg):
            bad.update_front({"tr_points": torch.zeros(2, 64, 3)})
    ct = ldt_amd.CompletionCompressorTrainer(cfg, ldt_amd.Compressor(cfg.compressor), "cpu")
    with pytest.raises(NotImplementedError, match="CompletionCompressorTrainer.update_front.*CompressorTrainer alone"):
        ct.update_front({"tr_points": torch.zeros(2, 64, 3)})
    with pytest.raises(NotImplementedError, match="CompressorTrainer.update: training \\(optimizer step, backward\\) is not on this path"):
        tr.update({})                                                    # update and compute_loss keep refusing, with their messages
    with pytest.raises(NotImplementedError, match="CompressorTrainer.compute_loss: its EMD_loss term"):
        tr.compute_loss(None, None)


# ------------------------------------------------------------------------------------------------- the references against autograd
def test_bn_references_equal_torch_batchnorm1d_in_training_mode():
    M, C = 37, 11
    c = fc.bn_case(M, C, seed=1)
    bn = torch.nn.BatchNorm1d(C).double()
    with torch.no_grad():
        bn.weight.copy_(c["gamma"]); bn.bias.copy_(c["beta"]); bn.running_mean.copy_(c["running_mean"]); bn.running_var.copy_(c["running_var"])
    bn.train()
    x = c["x"].double().requires_grad_(True)
    y = torch.relu(bn(x))
    y.backward(c["dy"].double())
    ref, _ = fc.bn_stats_ref(c["x"], c["running_mean"], c["running_var"])
    assert float((ref["running_mean"] - bn.running_mean).abs().max()) <= 1e-14 and float((ref["running_var"] - bn.running_var).abs().max()) <= 1e-13
    assert int(bn.num_batches_tracked) == 1
    stats = torch.stack([ref["mean"], ref["rstd"]])                       # float64 statistics: the references then ARE the module
    yr, _ = fc.bn_relu_fwd_ref(c["x"].double(), stats, c["gamma"], c["beta"], False)
    assert float((yr - y.detach()).abs().max()) <= 1e-13
    (dx, dg, db), _ = fc.bn_relu_bwd_ref(c["dy"], c["x"].double(), stats, c["gamma"], c["beta"], mask=y.detach() > 0)
    for got, want in ((dx, x.grad), (dg, bn.weight.grad), (db, bn.bias.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_group_normalize_bwd_reference_equals_autograd():
    for B, n, S, k, D in fc.GNB_CASES[:3]:
        c = fc.gnb_case(B, n, S, k, D)
        feat = c["feat"].double().requires_grad_(True)
        al = c["alpha"].double().requires_grad_(True)
        be = torch.zeros(D + 3, dtype=torch.float64, requires_grad=True)
        U = fc.group_forward64(feat, c["xyz"].double(), c["fi"], c["ki"], al, be)
        (U * c["dU"].double().view(B, S, k, -1)).sum().backward()
        ref, tol = fc.group_normalize_bwd_ref(c)
        for got, want, nm in zip(ref, (al.grad, be.grad, feat.grad), ("dalpha", "dbeta", "dfeat")):
            assert float((got - want).abs().max()) <= 1e-11 * float(want.abs().max()), (nm, B, n, S, k, D)
        assert bool((ref[2][:, c["none"]] == 0).all()) and bool((tol[2][:, c["none"]] == 0).all())
        for f in fc.GNB_FAULTS:                                          # each planted fault is far outside the bound
            bad, _ = fc.group_normalize_bwd_ref(c, fault=f)
            assert max(fc.worst_ratio(b.float(), r, t.clamp_min(1e-300)) for b, r, t in zip(bad, ref, tol)) > 3.0, (f, B, n, S, k, D)


def test_maxpool_reference_first_index_and_its_backward():
    G, n, C = 6, 5, 14
    x = fc.maxpool_case(G, n, C, seed=2)
    out, arg = fc.maxpool_argmax_ref(x, G, n)
    vals, idx = x.view(G, n, C).max(1)                                   # torch on the CPU: the first index on equal values
    assert torch.equal(out, vals) and torch.equal(arg.long(), idx)
    last = fc.maxpool_argmax_ref(x, G, n, last_wins=True)[1]
    assert not torch.equal(last, arg)                                    # the planted fault is visible: ties exist
    g = torch.Generator().manual_seed(3)
    d_out = torch.randn(G, C, generator=g)
    ref = fc.maxpool_relu_bwd_ref(d_out, out, arg, n)
    assert not torch.equal(fc.maxpool_relu_bwd_ref(d_out, out, last, n), ref)
    assert float(ref.view(G, n, C).sum(1).sub(torch.where(out > 0, d_out, torch.zeros(()))).abs().max()) == 0
    assert bool((ref.view(G, n, C)[:, :, 1::7] == 0).all()) and bool((out[:, 1::7] == 0).all())   # the all-zero cells pass nothing


# ------------------------------------------------------------------------------------------------- the emulation and the planted faults
def _bn_ratios(c, e):
    st = e["stats"]
    ref, tol = fc.bn_stats_ref(c["x"], c["running_mean"], c["running_var"])
    out = {k: fc.worst_ratio(e[k], ref[k], tol[k]) for k in ref}
    good = fc.bn_emulate(c)["stats"]                                      # the later stages are judged on the CORRECT statistics' references
    y, ty = fc.bn_relu_fwd_ref(c["x"], good, c["gamma"], c["beta"], False)
    out["y"] = fc.worst_ratio(e["y"], y, ty) if torch.equal(st, good) else 0.0
    (dx, dg, db), (tx, tg, tb) = fc.bn_relu_bwd_ref(c["dy"], c["x"], good, c["gamma"], c["beta"])
    if torch.equal(st, good):
        out.update({"dx": fc.worst_ratio(e["dx"], dx, tx), "dgamma": fc.worst_ratio(e["dgamma"], dg, tg), "dbeta": fc.worst_ratio(e["dbeta"], db, tb)})
    return out


@pytest.mark.parametrize("M,C", fc.BN_CASES)
def test_bn_emulation_sits_inside_the_bounds(M, C):
    c = fc.bn_case(M, C)
    r = _bn_ratios(c, fc.bn_emulate(c))
    print("fp32 emulation (%d, %d): %s" % (M, C, "  ".join("%s %.3f" % kv for kv in r.items())))
    assert max(r.values()) < 1.0, r
    ref, tol = fc.bn_stats_ref(c["x"])
    assert float((tol["rstd"] / ref["rstd"]).max()) < 2.0 ** -22                                   # bounds of a few roundings, not loose ones


def test_bn_planted_faults_leave_the_bounds():
    worst = {f: 0.0 for f in fc.BN_FAULTS}
    for M, C in fc.BN_CASES:
        c = fc.bn_case(M, C)
        for f in fc.BN_FAULTS:
            if f == "fp32 running sums" and M != 70000:
                continue
            if f != "fp32 running sums" and M == 70000:
                continue
            worst[f] = max(worst[f], max(_bn_ratios(c, fc.bn_emulate(c, fault=f)).values()))
    print("planted faults, worst err / tol over the table: " + "; ".join("%s %.3g" % kv for kv in worst.items()))
    assert all(v > 3.0 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------- the restated front
def _front_setup(tiny_cfg, seed=0, B=3):
    from oracle import ldt_oracle as O
    c = copy.deepcopy(tiny_cfg.compressor)
    torch.manual_seed(seed)
    m = _compressor(tiny_cfg)
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    cloud = torch.randn(B, c.outsize, 3, generator=g) * 0.5
    fi = O.fps(cloud, c.z_scales)
    ki = O.knn(c.outsize // c.z_scales * 2, cloud, O.gather(cloud, fi))
    d_tok = torch.randn(B, c.z_scales, c.hidden_dim, generator=g) * 0.1
    d_pos = torch.randn(B, c.p_dim, generator=g) * 0.1
    return c, m, init, cloud, fi, ki, d_tok, d_pos


def test_the_restated_front_is_the_module_in_training_mode(tiny_cfg):
    """Against torch's own layers: Conv1d / BatchNorm1d (training) / ReLU / max, built from the same state_dict, under autograd."""
    import torch.nn as nn
    c, m, init, cloud, fi, ki, d_tok, d_pos = _front_setup(tiny_cfg)
    grads, tok, pos, sel, bns = fc.front_step(init, c, cloud, fi, ki, d_tok, d_pos, torch.float64)
    D, T, B = c.hidden_dim, c.z_scales, cloud.shape[0]
    k = ki.shape[2]
    sd = {n: v.double() for n, v in init.items()}
    leaves = {n: sd[n].clone().requires_grad_(True) for n in fc.front_names(init)}
    P = lambda n: leaves[n]
    conv = lambda x, p: nn.functional.conv1d(x, P(p + ".weight"), P(p + ".bias"))
    bn = lambda x, p: nn.functional.batch_norm(x, None, None, P(p + ".weight"), P(p + ".bias"), training=True, eps=1e-5)
    x = cloud.double().transpose(1, 2)                                    # channels first, as the reference runs
    feat = conv(x, "input").transpose(1, 2)
    U = fc.group_forward64(feat, cloud.double(), fi, ki, P("group.affine_alpha").reshape(-1), P("group.affine_beta").reshape(-1))
    u = U.reshape(B * T, k, -1).transpose(1, 2)                           # [B T, 2 D + 3, k]
    ex = "group.extraction."
    # BatchNorm1d over (batch = B T groups, length = k): the statistics run over all B T k rows
    h1 = torch.relu(bn(conv(u, ex + "transfer.net.0"), ex + "transfer.net.1"))
    r = torch.relu(bn(conv(h1, ex + "operation.0.net1.0"), ex + "operation.0.net1.1"))
    h2 = torch.relu(conv(r, ex + "operation.0.net2.0") + h1)
    tk = h2.max(2).values.view(B, T, D)
    ctr = kc._take(cloud.double(), fi.long()).transpose(1, 2)
    a1 = torch.relu(bn(conv(ctr, "pos_embedding.conv1"), "pos_embedding.bn1"))
    a2 = torch.relu(bn(conv(a1, "pos_embedding.conv2"), "pos_embedding.bn2"))
    ps = nn.functional.linear(a2.max(2).values, P("pos_embedding.fc.weight"), P("pos_embedding.fc.bias"))
    assert rel_mse(tok, tk.detach()) < 1e-24 and rel_mse(pos, ps.detach()) < 1e-24
    torch.autograd.backward([tk, ps], [d_tok.double(), d_pos.double()])
    # the bias in front of a training-mode BatchNorm has an analytically zero gradient: rounding noise on both sides, held apart.  So have
    # affine_beta and the input conv's bias: each shifts every row of some columns of U by one constant (the bias cancels in g - anchor and
    # stays in the anchor columns), which the transfer conv turns into a per-channel constant that its BatchNorm removes
    dead = fc.FRONT_DEAD
    per = {n: rel_mse(grads[n], leaves[n].grad) for n in leaves if n not in dead}
    worst = max(per.values())
    assert worst <= 1e-20, {n: v for n, v in per.items() if v > 1e-20}
    print("restated front against torch's layers under autograd: worst gradient rel-MSE %.3e" % worst)
    assert worst <= 1e-20
    for n, live in dead.items():
        assert float(grads[n].abs().max()) <= 1e-12 * float(grads[live].abs().max()), n
    after = fc.running_after(init, bns)
    assert all(int(after[p + ".num_batches_tracked"]) == 1 for p in bns) and len(bns) == 4


def test_the_restated_front_differentiates_at_pinned_selections(tiny_cfg):
    """Pinned to the bf16 twin's selections the float64 gradients move away from the free ones by the flipped cells alone, and the twin
    pinned to ITS OWN selections is unchanged; the twin's selection shares stay inside the caps the GPU test holds the device to."""
    c, m, init, cloud, fi, ki, d_tok, d_pos = _front_setup(tiny_cfg)
    free, tok, pos, sel, _ = fc.front_step(init, c, cloud, fi, ki, d_tok, d_pos, torch.float64)
    twin, _, _, tsel, _ = fc.front_step(init, c, cloud, fi, ki, d_tok, d_pos, torch.float32, twin=True)
    again, _, _, asel, _ = fc.front_step(init, c, cloud, fi, ki, d_tok, d_pos, torch.float32, sel=tsel, twin=True)
    assert all(torch.equal(asel[k], tsel[k]) for k in fc.FRONT_SELECTIONS) and all(torch.equal(again[n], twin[n]) for n in twin)
    shares = fc.selection_shares(sel, tsel)
    print("bf16 twin against float64, selection shares: " + "  ".join("%s %.4f" % kv for kv in shares.items()))
    assert shares["arg"] <= 0.02 and max(shares[k] for k in ("mask1", "mask2", "mask3")) <= 0.01
    pinned, ptok, _, psel, _ = fc.front_step(init, c, cloud, fi, ki, d_tok, d_pos, torch.float64, sel=tsel)
    assert all(torch.equal(psel[k], tsel[k]) for k in fc.FRONT_SELECTIONS)
    names = [n for n in free if n not in fc.FRONT_DEAD]
    e_free = max(rel_mse(twin[n], free[n]) for n in names)
    e_pin = max(rel_mse(twin[n], pinned[n]) for n in names)
    print("twin against float64, worst gradient rel-MSE: free autograd %.3e, at the twin's selections %.3e" % (e_free, e_pin))
    assert e_pin <= e_free
