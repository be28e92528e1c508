"""CPU (no GPU needed): the encoder training step's host side (ldt_amd/compressor_train.py: EncoderTrainStep, encoder_parameters,
refuse_untrainable_encoder; CompressorTrainer.update_encoder; Compressor.front), the ActNorm backward's entry point (ldt_actnorm_bwd:
csrc/actnorm.hip) and the helpers of tests/encoder_train_checks.py.

  * ldt_actnorm_bwd is in the header, in the binding's table and in the built library; the ABI stays 26; its argument errors come back as
    LDT_EARG with a message: no launch
  * encoder_parameters on the tiny and on the shipped shape is the expected name list, disjoint from topdown_parameters; together with the
    frozen names (input, group, pos_embedding) the two lists cover named_parameters exactly
  * every refusal of refuse_untrainable_encoder fires on CPU parameters with its reason; `ActNorm: ~` is covered
  * update_encoder on a CPU device raises RuntimeError with nothing allocated; the completion trainer refuses; update / compute_loss keep
    their messages
  * the float64 restatement (encoder_train_checks.chain_step) reproduces tests/golden/encoder_train_tiny.npz: gradients <= 1e-9 rel-MSE,
    loss 1e-6 relative
  * the fp32 emulation of the ActNorm backward sits inside the float64 reference's bound on every case of the table, and each planted
    fault leaves it by more than 3 x the bound on some case: the wrong sign on dshift, x instead of z in dlog_scale, exp(+log_scale), a
    dropped last sample, fp32 running sums at B = 700

Before the step existed every test here ended at the missing symbol, attribute or helper."""
import copy
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import encoder_train_checks as ec
from conftest import GOLDEN, rel_mse


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib
    return _lib


def golden():
    z = np.load(os.path.join(GOLDEN, "encoder_train_tiny.npz"))
    return {k: (torch.from_numpy(np.asarray(z[k])) if z[k].dtype.kind in "fiu" else z[k]) for k in z.files}


def digest(t):                                                           # tools/gen_decoder_train_golden.py
    t = torch.as_tensor(t).detach().double().cpu().reshape(-1)
    return torch.stack([t.sum(), (t * t).sum(), (t * torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64))).sum()])


def same_digest(got, want, numel):
    return float((got - want).abs().max()) <= 1e-9 * (float(want[1]) * numel) ** 0.5 + 1e-300


def _compressor(tiny_cfg, **kw):
    import ldt_amd
    c = copy.deepcopy(tiny_cfg.compressor)
    for k, v in kw.items():
        setattr(c, k, v)
    return ldt_amd.Compressor(c)


def test_actnorm_bwd_is_declared_bound_and_built(built):
    _lib = built
    src = open(_lib._HERE + "/../include/ldt_hip.h").read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    params = [p.strip() for p in re.search(r"\bint ldt_actnorm_bwd\s*\(([^)]*)\)", decl).group(1).split(",")]
    assert [p.split()[-1] for p in params] == ["dz", "z", "log_scale", "B", "per_sample", "dx", "dshift", "dlog_scale", "stream"]
    kinds = {"int64_t": ctypes.c_int64}
    assert _lib.SIGNATURES["ldt_actnorm_bwd"] == [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
    assert "ldt_actnorm_bwd: backward of ldt_actnorm (model/layers.py:103-107" in src
    assert _lib.ABI_VERSION == 26 and _lib.lib().ldt_abi_version() == 26 and "#define LDT_ABI_VERSION 26" in src
    assert hasattr(_lib.lib(), "ldt_actnorm_bwd")


def test_actnorm_bwd_returns_argument_errors_before_any_launch(built):
    f = built.lib().ldt_actnorm_bwd
    err = built.lib().ldt_last_error
    ok = [16, 16, 16, 2, 8, 16, 16, 16, None]
    for i in (0, 2, 5):                                                  # dz, log_scale, dx
        a = list(ok)
        a[i] = None
        assert f(*a) == -1 and b"actnorm_bwd: null pointer" in err(), i
    a = list(ok)
    a[1] = None                                                          # z is read for dlog_scale
    assert f(*a) == -1 and b"dlog_scale needs z" in err()
    for B, per in ((0, 8), (-3, 8), (2, 0), (2, -1)):
        a = list(ok)
        a[3], a[4] = B, per
        assert f(*a) == -1 and b"B %d, per_sample %d" % (B, per) in err()


def test_ops_actnorm_bwd_checks_its_arguments_and_has_no_fallback():
    from ldt_amd import ops
    from ldt_amd._lib import LdtHipError
    assert list(inspect.signature(ops.actnorm_bwd).parameters) == ["dz", "z", "log_scale", "B", "dx", "dshift", "dlog_scale", "want_sums"]
    dz, z, ls = torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(8)
    with pytest.raises(LdtHipError, match="dz must be a device tensor.*no CPU fallback"):
        ops.actnorm_bwd(dz, z, ls, 2)
    with pytest.raises(LdtHipError, match="no CPU fallback"):            # (the shape errors behind it: test_gpu_actnorm_bwd.py)
        ops.actnorm_bwd(dz, z, ls, 2, dx=dz, want_sums=False)


def expected_names(L, E):
    blk = ["fc_q.weight", "fc_q.bias", "fc_kv.weight", "fc_kv.bias", "fc_o.weight", "fc_o.bias", "adaLN.1.weight", "adaLN.1.bias",
           "mlp.fc.0.0.weight", "mlp.fc.0.0.bias", "mlp.out.weight", "mlp.out.bias"]
    out = ["conv_in.shift", "conv_in.log_scale"]
    for i in range(L):
        for k in range(E):
            out += ["encoder.%d.atts.%d.%s" % (i, k, leaf) for leaf in blk]
        out += ["encoder.%d.conv_out.%s" % (i, leaf) for leaf in ("adaLN.1.weight", "adaLN.1.bias", "ln.weight", "ln.bias")]
    return out


@pytest.mark.parametrize("shape", ["tiny", "shipped"])
def test_encoder_parameters_are_the_encoder(tiny_cfg, shape):
    from ldt_amd.compressor_train import encoder_parameters, topdown_parameters
    kw = {} if shape == "tiny" else dict(hidden_dim=128, num_heads=4, n_layers=6, encoder_layers=2, p_dim=256, z_scales=32, z_dim=20)
    m = _compressor(tiny_cfg, **kw)
    names = [n for n, _ in encoder_parameters(m)]
    every = [n for n, _ in m.named_parameters()]
    assert names == expected_names(m.n_layers, m.encoder_layers)
    assert names == [n for n in every if n in set(names)]                # module order
    top = [n for n, _ in topdown_parameters(m)]
    assert not set(names) & set(top)
    frozen = [n for n in every if n not in set(names) and n not in set(top)]
    assert frozen and all(n.startswith(("input.", "group.", "pos_embedding.")) for n in frozen), frozen
    assert sorted(names + top + frozen) == sorted(every) and len(names) + len(top) + len(frozen) == len(every)
    assert all(p is dict(m.named_parameters())[n] for n, p in encoder_parameters(m))
    if shape == "tiny":
        g = golden()
        assert names == [str(n) for n in g["encoder_names"]] and top == [str(n) for n in g["topdown_names"]]
    # without ActNorm the list starts at the first block
    m = _compressor(tiny_cfg, ActNorm=None, **kw)
    assert [n for n, _ in encoder_parameters(m)] == expected_names(m.n_layers, m.encoder_layers)[2:]


def test_refuse_untrainable_encoder_names_each_reason(tiny_cfg):
    from ldt_amd.compressor_train import EncoderTrainStep, refuse_untrainable_encoder
    refuse_untrainable_encoder(_compressor(tiny_cfg))                    # the tiny config itself is covered; parameters on the CPU
    refuse_untrainable_encoder(_compressor(tiny_cfg, ActNorm=None))      # `ActNorm: ~`: the step simply has no ActNorm
    for kw, msg in ((dict(pos_embedding="mlp"), "pos_embedding: mlp.*per-token"),
                    (dict(class_condition=True, num_categorys=3), "class_condition"),
                    (dict(AdaLN=False), "AdaLN: False"),
                    (dict(norm="group_norm"), "norm='group_norm'.*layer_norm"),
                    (dict(encoder_dropout_p=0.1), "encoder_dropout_p=0.1"),
                    (dict(num_heads=4), "32-wide attention heads.*hidden 64 / 4 heads"),
                    (dict(z_scales=520), "encoder with 520 tokens.*1 <= Nq, Nk <= 512")):
        with pytest.raises(NotImplementedError, match=msg):
            EncoderTrainStep(_compressor(tiny_cfg, **kw))
    m = _compressor(tiny_cfg)
    with pytest.raises(NotImplementedError, match="encoder with 513 tokens"):
        refuse_untrainable_encoder(m, tokens=513)
    refuse_untrainable_encoder(m, tokens=512)
    assert EncoderTrainStep.MAX_TOKENS == 512
    step = EncoderTrainStep(m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        step.forward(torch.zeros(2, 8, 64), torch.zeros(2, 32))
    with pytest.raises(RuntimeError, match="before forward"):
        step.backward([torch.zeros(2, 8, 64)] * 3)
    assert list(inspect.signature(EncoderTrainStep.forward).parameters) == ["self", "tokens", "pos"]
    assert list(inspect.signature(EncoderTrainStep.backward).parameters) == ["self", "d_enc_out"]


def test_update_encoder_on_the_cpu_has_no_fallback_and_allocates_nothing(tiny_cfg):
    import ldt_amd
    tr = ldt_amd.CompressorTrainer(tiny_cfg, ldt_amd.Compressor(tiny_cfg.compressor), "cpu")
    assert tr.kl_weight is None and tr.encoder_optimizer is None and tr.last_tokens_grad is None and tr.last_pos_grad is None
    with pytest.raises(ValueError, match="update_encoder: cfg.opt.kl_weight is not set"):
        tr.update_encoder({"tr_points": torch.zeros(2, 64, 3)})
    cfg = copy.deepcopy(tiny_cfg)
    cfg.opt.kl_weight = 0.5
    tr = ldt_amd.CompressorTrainer(cfg, ldt_amd.Compressor(cfg.compressor), "cpu")
    before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
    with pytest.raises(RuntimeError, match="update_encoder: device cpu; the HIP path has no CPU fallback"):
        tr.update_encoder({"tr_points": torch.zeros(2, 64, 3)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.update_encoder({"tr_points": torch.zeros(2, 64, 3)}, tokens=torch.zeros(2, 8, 64), pos=torch.zeros(2, 32), post_noise=[torch.zeros(2, 8, 40)] * 3)
    assert tr.encoder_optimizer is None and tr.topdown_optimizer is None and tr.optimizer is None and tr.itr == 0
    assert all(p.grad is None for p in tr.model.parameters()) and float(tr.model.conv_in.initialized) == 0
    assert all(torch.equal(p, before[n]) for n, p in tr.model.named_parameters())
    ct = ldt_amd.CompletionCompressorTrainer(cfg, ldt_amd.Compressor(cfg.compressor), "cpu")
    with pytest.raises(NotImplementedError, match="CompletionCompressorTrainer.update_encoder.*CompressorTrainer alone"):
        ct.update_encoder({"tr_points": torch.zeros(2, 64, 3)})
    with pytest.raises(NotImplementedError, match="CompressorTrainer.update: training \\(optimizer step, backward\\) is not on this path"):
        tr.update({})                                                    # update and compute_loss keep refusing, with their messages
    with pytest.raises(NotImplementedError, match="CompressorTrainer.compute_loss: its EMD_loss term"):
        tr.compute_loss(None, None)
    kw = [p.name for p in inspect.signature(ldt_amd.CompressorTrainer.update_encoder).parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert kw == ["tokens", "pos", "post_noise"]
    bad = ldt_amd.CompressorTrainer(cfg, _compressor(cfg, pos_embedding="mlp"), "cpu")
    with pytest.raises(NotImplementedError, match="pos_embedding: mlp"):
        bad.update_encoder({"tr_points": torch.zeros(2, 64, 3)})
    with pytest.raises(RuntimeError, match="Compressor.front: parameters on cpu"):
        tr.model.front(torch.zeros(2, 64, 3))
    assert list(inspect.signature(ldt_amd.Compressor.front).parameters) == ["self", "x", "label"]


def test_the_float64_restatement_reproduces_the_fixture(tiny_cfg):
    import ldt_amd
    g = golden()
    c = copy.deepcopy(tiny_cfg.compressor)
    torch.manual_seed(int(g["seed"]))
    model = ldt_amd.Compressor(c)
    model.init()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    shift, log_scale = ec.perturb_actnorm(init)
    assert torch.equal(shift, g["actnorm_shift"]) and torch.equal(log_scale, g["actnorm_log_scale"])
    assert float(shift.abs().max()) > 0 and float(log_scale.abs().max()) > 0                 # NOT the identity of init()
    for k, v in init.items():
        assert same_digest(digest(v), g["init_digest::" + k], v.numel()), "initial weights differ from the fixture's: " + k
    enc_names, top_names = [str(n) for n in g["encoder_names"]], [str(n) for n in g["topdown_names"]]
    names = enc_names + top_names
    L = c.n_layers
    post_noise = [g["post_noise.%d" % i] for i in range(L)]
    ref, loss, pts, all_eps, enc_out = ec.chain_step(init, c, names, g["tokens"], g["pos"], post_noise, g["target"], torch.float64, float(g["kl_weight"]))
    assert abs(loss[0] - float(g["loss"])) <= 1e-6 * abs(float(g["loss"])) and abs(loss[1] - float(g["kl_loss"])) <= 1e-6 * abs(float(g["kl_loss"]))
    assert abs(loss[2] - float(g["rec_loss"])) <= 1e-6 * float(g["rec_loss"])
    assert rel_mse(pts, g["set"]) < 1e-10 and rel_mse(all_eps, g["all_eps"]) < 1e-10
    worst = 0.0
    for k in ["d_tokens", "d_pos"] + ["d_enc_out.%d" % i for i in range(L)]:
        worst = max(worst, rel_mse(ref[k], g[k]))
    for i in range(L):
        assert rel_mse(enc_out[i], g["enc_out.%d" % i]) < 1e-10
    for n in names:
        d, w = digest(ref[n]), g["grad_digest::" + n]                    # (float64 against the captured fp32 gradient: rel-MSE ~1e-12)
        assert abs(float(d[1] - w[1])) <= 1e-5 * float(w[1]) and abs(float(d[2] - w[2])) <= 1e-5 * (float(w[1]) * ref[n].numel()) ** 0.5, n
        if "grad::" + n in g:
            worst = max(worst, rel_mse(ref[n], g["grad::" + n]))
    print("float64 restatement against the fixture: worst gradient rel-MSE %.3e (the generator's own figure: %.3e)" % (worst, float(g["oracle_grad_relmse"])))
    assert worst <= 1e-9 and float(g["oracle_grad_relmse"]) <= 1e-10
    assert sum(("grad::" + n) in g for n in enc_names) >= 20
    # the encoder alone from the fixture's d_enc_out gives the chain's encoder gradients: the chain rule, restated
    alone, _ = ec.encoder_step(init, c, enc_names, g["tokens"], g["pos"], [g["d_enc_out.%d" % i] for i in range(L)], torch.float64)
    for n in enc_names + ["d_tokens", "d_pos"]:
        assert rel_mse(alone[n], ref[n]) <= 1e-9, n


@pytest.mark.parametrize("B,per", ec.ANB_CASES)
def test_actnorm_bwd_emulation_sits_inside_the_bound(B, per):
    c = ec.actnorm_case(B, per)
    ref, tol = ec.actnorm_bwd_ref(c["dz"], c["z"], c["log_scale"])
    r = ec.actnorm_worst(ec.actnorm_bwd_emulate(c["dz"], c["z"], c["log_scale"]), ref, tol, "fp32 emulation (%d, %d)" % (B, per))
    assert max(r) < 1.0
    # a bound of a few fp32 roundings, not a loose one
    assert float((tol[0] / ref[0].abs().clamp_min(1e-30)).max()) < 4 * 2.0 ** -23
    assert float((tol[2] / ref[2].abs().clamp_min(1e-30)).median()) < 2.0 ** -23


def test_actnorm_bwd_reference_equals_autograd():
    c = ec.actnorm_case(5, 24, ls_max=3.0)
    x = c["x"].double().requires_grad_(True)
    sh, ls = c["shift"].double().requires_grad_(True), c["log_scale"].double().requires_grad_(True)
    z = (x - sh) * torch.exp(-ls)
    z.backward(c["dz"].double())
    ref, _ = ec.actnorm_bwd_ref(c["dz"], z.detach(), c["log_scale"])
    for got, want in zip(ref, (x.grad, sh.grad, ls.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_actnorm_bwd_planted_faults_leave_the_bound():
    """Each fault is beyond 3 x the bound on some case of the table."""
    worst = {f: 0.0 for f in ec.ANB_FAULTS}
    for B, per in ec.ANB_CASES:
        if B * per > 1 << 17:                                            # (the large cases add nothing here; 700 rows is where fp32 sums show)
            continue
        c = ec.actnorm_case(B, per)
        ref, tol = ec.actnorm_bwd_ref(c["dz"], c["z"], c["log_scale"])
        for f in ec.ANB_FAULTS:
            worst[f] = max(worst[f], ec.actnorm_ratio(ec.actnorm_bwd_emulate(c["dz"], c["z"], c["log_scale"], x=c["x"], fault=f), ref, tol))
            if f == "fp32 running sums" and B == 700:
                at700 = ec.actnorm_ratio(ec.actnorm_bwd_emulate(c["dz"], c["z"], c["log_scale"], x=c["x"], fault=f), ref, tol)
    print("planted faults, worst err / tol over the table: " + "; ".join("%s %.3g" % kv for kv in worst.items()))
    assert all(v > 3.0 for v in worst.values()), worst
    assert at700 > 3.0
