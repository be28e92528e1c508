"""GPU (-m gpu): a whole Score backward audited call by call, at ragged shapes (tests/train_tape.py; its teeth are shown on the CPU by
test_train_tape_host.py).

test_gpu_train_kernels.py holds every backward kernel alone, on fresh contiguous operands; test_gpu_train.py holds whole steps at one friendly
shape (T = 8) by per-tensor rel-MSE.  Inside a step the kernels run on operands neither gives them — column blocks of `dmod` with row stride
n_mod, row ranges of the flat gradient, the strided [dk | dv] half of dqkv, a dX accumulated into three times per block, the raw
[B][H][T][64] dO, a pad64(M) contraction whose last tile is partial — and `ScoreTrainStep.backward` is 80 lines of offsets and saved-tensor
choices.  Here `ScoreTrainStep` is driven directly (forward, ops.dsm_loss_bwd, backward: T is free) with `ldt_amd.train.ops` replaced by a
recording proxy, and
  * every recorded call is held per element against float64 from ITS OWN recorded operands, with the bounds of kernel_checks.py that the
    stand-alone tests use (teacher forcing: the depth of the network enters no bound), in-place accumulations as after - before, and the
    storage around every strided destination unchanged;
  * every operand is bit-equal to what the reference's block says it must be (train_tape.audit_wiring's table), and every parameter's final
    .grad to the output of the call that owns it;
  * the final gradients and the forward's output are held to the oracle's float64 autograd by the yardstick of test_gpu_train.py: rel-MSE
    <= 2 x a bf16 twin's (the same oracle under CPU autocast, computed here), per tensor against max(the twin's for that tensor, the twin's
    over all), and over the concatenation.  The margin of 2 and its reason are stated at the top of test_gpu_train.py;
  * exact structure probes on the ragged case: sample isolation, absent classes, determinism.
Each case is run once and shared by the tests.  The largest err / tol per call kind and the twin ratios are printed (-s); DESIGN.md section 4.11
records them."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import train_tape as tt
from conftest import rel_mse

pytestmark = pytest.mark.gpu

_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_tapes():
    yield
    _RUNS.clear()


def run_case(tiny_cfg, name, edit=None, key=None):
    """One taped forward + backward of case `name` (cached under `key` or the name).  edit(dparams) -> the dparams handed to backward."""
    key = key or name
    if key in _RUNS:
        return _RUNS[key]
    import ldt_amd.train as train
    model, x, t, label, eta = tt.make_case(tiny_cfg.score, **tt.CASES[name])
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda()
    tt.flat_grads(model)
    tape = tt.Tape(train.ops)
    with pytest.MonkeyPatch.context() as mp:
        tt.install_ops(mp, tape)
        step = train.ScoreTrainStep(model)
        params = step.forward(x.cuda(), t.cuda(), None if label is None else label.cuda())
        S = tt.copy_saved(step.saved)
        tape.mark("backward")
        dparams = tape.dsm_loss_bwd(eta.cuda(), params)
        if edit is not None:
            dparams = edit(dparams)
        step.backward(dparams)
        assert step.saved is None
    torch.cuda.synchronize()
    r = dict(model=model, tape=tape, S=S, dparams=dparams, params=params.clone(), init=init, x=x, t=t, label=label, eta=eta,
             grads={n: p.grad.clone() for n, p in model.named_parameters()})
    _RUNS[key] = r
    return r


@pytest.mark.parametrize("name", list(tt.CASES))
def test_every_call_of_the_backward_within_its_own_bound(tiny_cfg, name):
    r = run_case(tiny_cfg, name)
    calls = r["tape"].since("backward")
    worst = tt.audit_numeric(calls)
    for kind in sorted(worst):
        print("train-tape %-7s %-32s max err/tol %.3f" % (name, kind, worst[kind]))
    nb = r["model"].num_blocks
    count = lambda k: sum(c.name == k for c in calls)
    assert count("layernorm_modulate_bwd") == 2 * nb + 1 and count("gate_residual_bwd") == 2 * nb and count("attention_bwd") == nb
    assert count("wgrad") == 5 * nb + 2 and count("dgrad") == 4 * nb + 1 and count("embedding_grad") == (r["label"] is not None)
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("name", list(tt.CASES))
def test_every_operand_is_what_the_reference_block_says(tiny_cfg, name):
    r = run_case(tiny_cfg, name)
    for n, p in r["model"].named_parameters():                              # (a later run on the same model rewrites .grad: the audit gets this run's)
        p.grad.copy_(r["grads"][n])
    placed = tt.audit_wiring(r["tape"].since("backward"), r["model"], r["S"], r["dparams"])
    print("train-tape %-7s wiring: %d calls placed, every link and every final .grad bit-equal" % (name, placed))


def oracle_run(r, cfg, dtype, autocast=False):
    """oracle.score_forward + autograd of the step's loss on the CPU -> (params, {name: grad})."""
    from oracle import ldt_oracle as O
    sd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in r["init"].items()}
    c = lambda v: v.to(dtype)
    with (torch.autocast("cpu", torch.bfloat16) if autocast else contextlib.nullcontext()):
        lab = None
        if r["label"] is not None:
            lab = O.linear(sd, "LabelEmbedding.mlp.2", F.silu(O.linear(sd, "LabelEmbedding.mlp.0", sd["LabelEmbedding.label_emb.weight"][r["label"]])))
        params = O.score_forward(sd, cfg, c(r["x"]), c(r["t"]), label_emb=lab)
        loss = ((c(r["eta"]) - params) ** 2).mean()
    loss.float().backward() if autocast else loss.backward()
    return params.detach(), {k: v.grad for k, v in sd.items()}


@pytest.mark.parametrize("name", list(tt.CASES))
def test_gradients_and_output_against_the_float64_oracle_at_the_twin_yardstick(tiny_cfg, name):
    r = run_case(tiny_cfg, name)
    cfg = r["model"].cfg
    names = [n for n, _ in r["model"].named_parameters()]
    p64, g64 = oracle_run(r, cfg, torch.float64)
    pt, gt = oracle_run(r, cfg, torch.float32, autocast=True)
    cat = lambda g: torch.cat([g[n].reshape(-1).double().cpu() for n in names])
    twin = {n: rel_mse(gt[n], g64[n]) for n in names}
    twin_all, twin_p = rel_mse(cat(gt), cat(g64)), rel_mse(pt, p64)
    e_p = rel_mse(r["params"].cpu(), p64)
    worst = 0.0
    for n in names:
        got = r["grads"][n]
        assert got.shape == g64[n].shape and bool(torch.isfinite(got).all()), n
        e, bar = rel_mse(got.cpu(), g64[n]), 2 * max(twin[n], twin_all)
        worst = max(worst, e / bar)
        assert e <= bar, "%s: gradient rel-MSE %.3e > %.3e (2 x the bf16 twin's)" % (n, e, bar)
    e_all = rel_mse(cat(r["grads"]), cat(g64))
    print("train-tape %-7s gradient rel-MSE, all parameters: %.3e = %.2f x the twin's %.3e; worst per-tensor ratio to its bar %.2f; "
          "params rel-MSE %.3e = %.2f x the twin's %.3e" % (name, e_all, e_all / twin_all, twin_all, worst, e_p, e_p / twin_p, twin_p))
    assert e_all <= 2 * twin_all
    assert e_p <= 2 * twin_p


# ------------------------------------------------------------------------------------------------ exact structure probes (zeros need no bound)
def test_a_gradient_in_one_sample_stays_in_that_sample(tiny_cfg):
    """dparams zero outside sample 1 of the ragged case (labels [2, 0, 2]): every recorded row of samples 0 and 2 — of dmod, dX, dh, dq, dk, dv
    and every other per-token gradient — is exactly 0, and so is every row of the label-embedding gradient except class 0's."""
    c = tt.CASES["ragged"]
    B, T = c["B"], c["T"]

    def only_sample_1(dp):
        dp = dp.clone()
        dp[0].zero_(); dp[2].zero_()
        return dp
    r = run_case(tiny_cfg, "ragged", edit=only_sample_1, key="ragged/sample 1")
    other_tokens = torch.ones(B * T, dtype=torch.bool, device="cuda")
    other_tokens[T:2 * T] = False
    seen = {"dmod": 0, "tokens": 0}
    for call in r["tape"].since("backward")[1:]:
        outs = [(k, d["after"].value) for k, d in call.inplace.items()] + [("output %d" % i, o.value) for i, o in enumerate(call.outs) if o is not None]
        for k, v in outs:
            if k in ("dshift", "dscale", "dgate"):
                assert v.shape[0] == B and float(v[[0, 2]].abs().max()) == 0.0 and float(v[1].abs().max()) > 0.0, "%s: %s" % (call, k)
                seen["dmod"] += 1
            elif v.dim() == 2 and v.shape[0] == B * T:
                assert float(v[other_tokens].abs().max()) == 0.0 and float(v[~other_tokens].abs().max()) > 0.0, "%s: %s" % (call, k)
                seen["tokens"] += 1
    nb = c["blocks"]
    assert seen["dmod"] == 6 * nb + 2 and seen["tokens"] >= 11 * nb + 3
    g = r["grads"]["LabelEmbedding.label_emb.weight"]
    assert float(g[1:].abs().max()) == 0.0 and float(g[0].abs().max()) > 0.0


def test_absent_classes_get_an_exactly_zero_embedding_gradient(tiny_cfg):
    g = run_case(tiny_cfg, "ragged")["grads"]["LabelEmbedding.label_emb.weight"]
    assert g.shape[0] == 4 and float(g[[1, 3]].abs().max()) == 0.0 and float(g[0].abs().max()) > 0.0 and float(g[2].abs().max()) > 0.0


def test_a_second_forward_and_backward_gives_the_same_bits(tiny_cfg):
    a, b = run_case(tiny_cfg, "ragged"), run_case(tiny_cfg, "ragged", key="ragged/again")
    assert torch.equal(a["params"], b["params"])
    for n in a["grads"]:
        assert torch.equal(a["grads"][n], b["grads"][n]), n


def test_more_than_512_tokens_is_refused_by_the_entry_point(tiny_cfg):
    """T = 520 is above ldt_attention_bwd's N <= 512: an argument check that returns a status before anything is launched.  The step must
    surface the entry point's message and leave no saved activations behind."""
    import ldt_amd.train as train
    from ldt_amd._lib import LdtHipError
    model, x, t, _, eta = tt.make_case(tiny_cfg.score, hidden=128, heads=2, blocks=1, B=1, T=520, classes=1, labels=None)
    model.cuda()
    tt.flat_grads(model)
    step = train.ScoreTrainStep(model)
    params = step.forward(x.cuda(), t.cuda())
    assert step.saved is not None
    with pytest.raises(LdtHipError, match=r"ldt_attention_bwd failed \(status -2\): attention_bwd: .*N 520 \(self-attention, N <= 512\)"):
        step.backward(train.ops.dsm_loss_bwd(eta.cuda(), params))
    assert step.saved is None
    torch.cuda.synchronize()
