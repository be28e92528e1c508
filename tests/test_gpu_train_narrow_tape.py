"""GPU (-m gpu): a whole Score backward at head widths 8, 16 and 32 audited call by call (tests/train_tape.py, imported as it is; the
attention call by kernel_checks.attn_bwd_ref at the call's own head width).

`ScoreTrainStep` is driven under train_tape.Tape as test_gpu_train_tape.py drives it, on the hybrid config's layout (hidden 128, 16 heads,
T = 32) and three more.  train_tape's own attention reference and its wiring table are written for 64-wide heads, so here
  * every recorded call of the backward is held per element by tt.check_call / tt.check_untouched, except attention_bwd, which gets the
    generalised bound (Dh for 64; P and dS rounded or not as the kernel for that width does) from that call's own recorded operands;
  * the attention call's links are checked by bit equality: q, k, v are the column blocks of the block's saved qkv, o the saved o, dO the
    output of fc_o's dgrad, head_dim = hidden / heads, and [dk | dv] and dq are the dY of fc_kv's and fc_q's weight-gradient calls (the
    rest of the wiring does not depend on the head width and stays held by test_gpu_train_tape.py);
  * gradients and the forward output are held to the float64 oracle at the yardstick stated at the top of test_gpu_train.py: rel-MSE
    <= 2 x a bf16 twin's, computed here;
  * on the ragged case: sample isolation and bit-equal repeats.
Each case is run once and shared.  The largest ratios are printed (-s); DESIGN.md section 4.13 records them."""
import pytest
import torch

import kernel_checks as kc
import narrow_bwd_checks as nb
import train_tape as tt
from conftest import rel_mse
from test_gpu_train_tape import oracle_run

pytestmark = pytest.mark.gpu

CASES = {
    "hybrid": dict(hidden=128, heads=16, blocks=2, B=3, T=32, classes=1, labels=None),       # the hybrid config's Score layout
    "ragged16": dict(hidden=128, heads=8, blocks=2, B=3, T=40, classes=4, labels=[2, 0, 2]),  # partial 16-row block, 32-step; absent classes
    "dh32": dict(hidden=128, heads=4, blocks=1, B=2, T=24, classes=1, labels=None),
    "one": dict(hidden=128, heads=16, blocks=1, B=1, T=40, classes=1, labels=None),           # one sample: rows_per_sample = M < 64
}
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
    model, x, t, label, eta = tt.make_case(tiny_cfg.score, **CASES[name])
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


def check_attention_call(call):
    a = call.arg
    B, H, N, Dh = a("B"), a("H"), a("N"), a("head_dim")
    ref, tol = kc.attn_bwd_ref(a("q"), a("k"), a("v"), a("o").reshape(B, H, N, Dh), a("do").reshape(B, H, N, Dh), B, H, N, N, Dh, nb.rounds(Dh))
    return {"attention_bwd " + k: kc.assert_elementwise(nb.heads(call.out(i), B, H, N, Dh), ref[k], tol[k], "%s, %s" % (call, k))
            for i, k in enumerate(("dq", "dk", "dv"))}


@pytest.mark.parametrize("name", list(CASES))
def test_every_call_of_the_backward_within_its_own_bound(tiny_cfg, name):
    r = run_case(tiny_cfg, name)
    calls = r["tape"].since("backward")
    worst = {}
    for call in calls:
        tt.check_untouched(call)
        for k, v in (check_attention_call(call) if call.name == "attention_bwd" else tt.check_call(call)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    for kind in sorted(worst):
        print("train-tape %-8s %-32s max err/tol %.3f" % (name, kind, worst[kind]))
    nblk = r["model"].num_blocks
    count = lambda k: sum(c.name == k for c in calls)
    assert count("layernorm_modulate_bwd") == 2 * nblk + 1 and count("gate_residual_bwd") == 2 * nblk and count("attention_bwd") == nblk
    assert count("wgrad") == 5 * nblk + 2 and count("dgrad") == 4 * nblk + 1 and count("embedding_grad") == (r["label"] is not None)
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_the_attention_call_is_wired_to_its_block(tiny_cfg, name):
    from ldt_amd.layers import conv_w
    r = run_case(tiny_cfg, name)
    m, S, calls = r["model"], r["S"], r["tape"].since("backward")
    for n, p in m.named_parameters():                                       # (a later run on the same model rewrites .grad)
        p.grad.copy_(r["grads"][n])
    D, H = m.hidden_size, m.num_heads
    B, T = S["B"], S["T"]
    W = tt.Wiring(calls)
    epi_bf16, _ = tt._epilogues()
    for l, (blk, sb) in enumerate(zip(m.Transformer, S["blocks"])):
        at = W.find("attention_bwd", lambda c: tt._eqflat(c.arg("o"), sb["o"]), "reads the saved attention output of block %d" % l)
        for i, nm in enumerate("qkv"):
            W.link(at, nm, sb["qkv"][:, i * D:(i + 1) * D].contiguous(), "columns [%d D, %d D) of the saved qkv of block %d" % (i, i + 1, l))
        for nm, v in (("B", B), ("H", H), ("N", T), ("head_dim", D // H)):
            W.link(at, nm, v, "%s = %d" % (nm, v))
        w_t = kc.transpose_cast_want(conv_w(blk.fc_o).detach())
        dg = W.find("dgrad", lambda c: tt._eq(c.arg("w_t"), w_t), "multiplies by the transposed weights of fc_o of block %d" % l)
        W.link(dg, "epilogue", epi_bf16, "the bf16 epilogue")
        W.link(at, "do", dg.result(), "the dgrad of fc_o of block %d, as the raw [B][H][T][Dh] buffer" % l, flat=True)
        dq, dk, dv = at.out(0), at.out(1), at.out(2)
        assert "out" not in at.inplace or tt._eq(at.after("out"), torch.cat([dq, dk, dv], 1)), "%s: dq | dk | dv are not the column blocks of its `out`" % at
        for layer, dy, what in ((blk.fc_q, dq, "dq"), (blk.fc_kv, torch.cat([dk, dv], 1), "[dk | dv]")):
            cw = W.dest("wgrad", "out", layer.weight.grad.view(layer.weight.shape[0], -1), "the weight .grad fed by %s of block %d" % (what, l))
            W.link(cw, "dy", dy, "%s of block %d" % (what, l))
    print("train-tape %-8s attention wiring: %d blocks, every link bit-equal" % (name, len(S["blocks"])))


@pytest.mark.parametrize("name", list(CASES))
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
    print("train-tape %-8s gradient rel-MSE, all parameters: %.3e = %.2f x the twin's %.3e; worst per-tensor ratio to its bar %.2f; "
          "params rel-MSE %.3e = %.2f x the twin's %.3e" % (name, e_all, e_all / twin_all, twin_all, worst, e_p, e_p / twin_p, twin_p))
    assert e_all <= 2 * twin_all
    assert e_p <= 2 * twin_p


def test_a_gradient_in_one_sample_stays_in_that_sample(tiny_cfg):
    """dparams zero outside sample 1 of the ragged case (labels [2, 0, 2]): every recorded row of samples 0 and 2 — of dmod, dX, dh, dq, dk, dv
    and every other per-token gradient — is exactly 0, and so is every row of the label-embedding gradient except class 0's."""
    c = CASES["ragged16"]
    B, T = c["B"], c["T"]

    def only_sample_1(dp):
        dp = dp.clone()
        dp[0].zero_(); dp[2].zero_()
        return dp
    r = run_case(tiny_cfg, "ragged16", edit=only_sample_1, key="ragged16/sample 1")
    other_tokens = torch.ones(B * T, dtype=torch.bool, device="cuda")
    other_tokens[T:2 * T] = False
    seen = {"dmod": 0, "tokens": 0, "attention": 0}
    per_channel = ("wgrad", "colsum", "sgemm", "transpose_cast_bf16", "embedding_grad")   # B T = 120 = z here: their rows are channels, not tokens
    for call in r["tape"].since("backward")[1:]:
        if call.name in per_channel:
            continue
        outs = [(k, d["after"].value) for k, d in call.inplace.items()] + [("output %d" % i, o.value) for i, o in enumerate(call.outs) if o is not None]
        for k, v in outs:
            if k in ("dshift", "dscale", "dgate"):
                assert v.shape[0] == B and float(v[[0, 2]].abs().max()) == 0.0 and float(v[1].abs().max()) > 0.0, "%s: %s" % (call, k)
                seen["dmod"] += 1
            elif v.dim() == 2 and v.shape[0] == B * T:
                assert float(v[other_tokens].abs().max()) == 0.0 and float(v[~other_tokens].abs().max()) > 0.0, "%s: %s" % (call, k)
                seen["tokens"] += 1
                seen["attention"] += call.name == "attention_bwd"
    nblk = c["blocks"]
    assert seen["dmod"] == 6 * nblk + 2 and seen["tokens"] >= 11 * nblk + 3 and seen["attention"] >= 3 * nblk
    g = r["grads"]["LabelEmbedding.label_emb.weight"]
    assert float(g[1:].abs().max()) == 0.0 and float(g[0].abs().max()) > 0.0


def test_a_second_forward_and_backward_gives_the_same_bits(tiny_cfg):
    a, b = run_case(tiny_cfg, "ragged16"), run_case(tiny_cfg, "ragged16", key="ragged16/again")
    assert torch.equal(a["params"], b["params"])
    for n in a["grads"]:
        assert torch.equal(a["grads"][n], b["grads"][n]), n
