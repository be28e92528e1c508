"""GPU (-m gpu): the Compressor's three training steps audited call by call (tests/compressor_tape.py; its teeth are shown on the CPU by
test_compressor_tape_host.py).

The stand-alone kernel tests hold every backward kernel alone on fresh dense operands, and test_gpu_decoder_train.py,
test_gpu_topdown_train.py and test_gpu_encoder_train.py hold the steps whole by per-tensor rel-MSE.  Inside a step the kernels run on
operands neither gives them: the column slice d_eps[:, z j : z (j + 1)] of row stride L z as ldt_sgemm's `out` and ldt_reparam_kl_bwd's
`d_eps`, the strided K | V halves of one buffer and the [dk | dv] destination, `.grad` views as `out` / `dshift` / `dscale`, column blocks
of dmod, a dX accumulated into by three kinds of call and in place by ldt_actnorm_bwd, the raw [B][H][Nq][32] dO, a backward K that is not
the forward's, ldt_sgemm at K = z + 1.  Here each step is driven with `ldt_amd.compressor_train.ops` replaced by a recording proxy, and
  * every recorded call of the backward, plus the centred-key calls of the forward, is held per element against float64 from ITS OWN
    recorded operands with the bound that holds the kernel alone (max err / tol <= 1), the storage around every destination unchanged, the
    call counts per kind as L, E and B give them;
  * every operand is bit-equal to what the reference says it must be (audit_decoder / audit_topdown / audit_encoder), every trained
    parameter's final .grad to what its owning call left, and in the chain TopDownTrainStep -> EncoderTrainStep every d_enc_out[i] handed
    on bit-equal;
  * the final gradients, d_eps, d_enc_out, d_tokens and d_pos are held to the float64 restatements at the yardstick of
    test_gpu_decoder_train.check_against_twin (rel-MSE <= 2 x the bf16 twin's; the margin of 2: the top of test_gpu_train.py), all three
    backward passes from ONE seeded upstream gradient;
  * exact probes: sample isolation, a prior row nobody keeps, determinism.
Each case is run once per module and shared.  The worst err / tol per call kind and the twin ratios are printed (-s); DESIGN.md section
4.18 records them."""
import pytest
import torch

import compressor_tape as cpt
import train_tape as tt

pytestmark = pytest.mark.gpu

_RUNS = {}
DEC_CASES = ("ragged", "odd")
ENC_CASES = ("ragged", "odd-enc", "odd-enc-plain")


@pytest.fixture(scope="module", autouse=True)
def _release_the_tapes():
    yield
    _RUNS.clear()


def _setup(tiny_cfg, name):
    import ldt_amd.compressor_train as ct
    case = cpt.make_case(tiny_cfg.compressor, **cpt.CASES[name])
    model = case["model"].cuda()
    tt.flat_grads(model)
    return ct, case, model, tt.Tape(ct.ops)


def _grads(params):
    return {n: p.grad.detach().clone() for n, p in params}


def run_decoder(tiny_cfg, name, edit=None, key=None):
    key = ("decoder", key or name)
    if key in _RUNS:
        return _RUNS[key]
    ct, case, model, tape = _setup(tiny_cfg, name)
    dset = case["d_set"].cuda() if edit is None else edit(case["d_set"].cuda())
    keep = case["keep"]
    with pytest.MonkeyPatch.context() as mp:
        tt.install_ops(mp, tape)
        step = ct.DecoderTrainStep(model)
        pts = step.forward(case["eps"].cuda(), num_points=case["N"], keep_mask=keep)
        S = cpt.copy_saved(step.saved)
        tape.mark("backward")
        d_eps = step.backward(dset)
        assert step.saved is None
    torch.cuda.synchronize()
    r = dict(case=case, model=model, tape=tape, S=S, dset=dset, d_eps=d_eps, pts=pts.clone(), grads=_grads(ct.decoder_parameters(model)))
    _RUNS[key] = r
    return r


def run_topdown(tiny_cfg, name, edit=None, key=None, kl_scale=None, then_encoder=False):
    key = ("chain" if then_encoder else "topdown", key or name)
    if key in _RUNS:
        return _RUNS[key]
    ct, case, model, tape = _setup(tiny_cfg, name)
    dset = case["d_set"].cuda() if edit is None else edit(case["d_set"].cuda())
    ks = case["kl_scale"] if kl_scale is None else kl_scale
    with pytest.MonkeyPatch.context() as mp:
        tt.install_ops(mp, tape)
        enc, enc_S = None, None
        if then_encoder:
            enc = ct.EncoderTrainStep(model)
            tape.mark("encoder forward")
            enc_out = enc.forward(case["tokens"].cuda(), case["pos"].cuda())
            enc_S = cpt.copy_saved(enc.saved)
        else:
            enc_out = [t.cuda() for t in case["enc_out"]]
        step = ct.TopDownTrainStep(model)
        tape.mark("forward")
        pts, all_eps, kls = step.forward(enc_out, [t.cuda() for t in case["post_noise"]], num_points=case["N"], keep_mask=case["keep"])
        S = cpt.copy_saved(step.saved)
        tape.mark("backward")
        d_enc = step.backward(dset, ks)
        d_enc_copy = [t.clone() for t in d_enc]
        r = dict(case=case, model=model, tape=tape, S=S, dset=dset, kl_scale=ks, d_eps=step.d_eps, d_enc=d_enc_copy, pts=pts.clone(),
                 grads=_grads(ct.topdown_parameters(model)), n_backward=None)
        if then_encoder:
            r["n_backward"] = len(tape.calls)
            tape.mark("encoder backward")
            d_tokens, d_pos = enc.backward(d_enc)
            r.update(enc_S=enc_S, d_tokens=d_tokens, d_pos=d_pos, enc_grads=_grads(ct.encoder_parameters(model)))
    torch.cuda.synchronize()
    _RUNS[key] = r
    return r


def run_encoder(tiny_cfg, name, edit=None, key=None):
    key = ("encoder", key or name)
    if key in _RUNS:
        return _RUNS[key]
    ct, case, model, tape = _setup(tiny_cfg, name)
    d_enc = [t.cuda() for t in case["d_enc"]]
    if edit is not None:
        d_enc = [edit(t) for t in d_enc]
    with pytest.MonkeyPatch.context() as mp:
        tt.install_ops(mp, tape)
        step = ct.EncoderTrainStep(model)
        outs = step.forward(case["tokens"].cuda(), case["pos"].cuda())
        S = cpt.copy_saved(step.saved)
        tape.mark("backward")
        d_tokens, d_pos = step.backward(d_enc)
        assert step.saved is None
    torch.cuda.synchronize()
    r = dict(case=case, model=model, tape=tape, S=S, d_enc=d_enc, d_tokens=d_tokens, d_pos=d_pos, outs=[o.clone() for o in outs],
             grads=_grads(ct.encoder_parameters(model)))
    _RUNS[key] = r
    return r


def _restore(model, grads):
    """A later run on the same parameters rewrites .grad: the audit gets this run's."""
    named = dict(model.named_parameters())
    for n, g in grads.items():
        named[n].grad.copy_(g)


def _report(what, worst):
    for kind in sorted(worst):
        print("compressor-tape %-22s %-34s max err/tol %.3f" % (what, kind, worst[kind]))
    assert max(worst.values()) <= 1.0


# ------------------------------------------------------------------------------------------------ numeric audit
@pytest.mark.parametrize("name", DEC_CASES)
def test_decoder_every_call_within_its_own_bound(tiny_cfg, name):
    r = run_decoder(tiny_cfg, name)
    calls = r["tape"].since("backward")
    cpt.assert_counts(calls, cpt.expected_counts("decoder", r["model"].n_layers), "decoder %s" % name)
    _report("decoder %s" % name, cpt.audit_numeric(calls))


@pytest.mark.parametrize("name", DEC_CASES)
def test_topdown_every_call_within_its_own_bound(tiny_cfg, name):
    r = run_topdown(tiny_cfg, name)
    m, tape = r["model"], r["tape"]
    calls = tape.since("backward")
    cpt.assert_counts(calls, cpt.expected_counts("topdown", m.n_layers), "top-down %s" % name)
    worst = cpt.audit_numeric(calls)
    fwd = tape.calls[tape.marks["forward"]:tape.marks["backward"]]
    _, n = cpt.audit_centred(fwd, cpt.centred_groups(m, r["S"], "topdown"), worst)
    assert n == m.n_layers * (2 * r["case"]["B"] + 1)                    # per level: B column sums, one sgemm, B per-sample GEMMs
    assert sum(c.name == "colsum" for c in fwd) == m.n_layers * r["case"]["B"]
    _report("top-down %s" % name, worst)


@pytest.mark.parametrize("name", ENC_CASES)
def test_encoder_every_call_within_its_own_bound(tiny_cfg, name):
    r = run_encoder(tiny_cfg, name)
    m, tape = r["model"], r["tape"]
    calls = tape.since("backward")
    cpt.assert_counts(calls, cpt.expected_counts("encoder", m.n_layers, m.encoder_layers, m.ActNorm is not None), "encoder %s" % name)
    worst = cpt.audit_numeric(calls)
    fwd = tape.calls[:tape.marks["backward"]]
    _, n = cpt.audit_centred(fwd, cpt.centred_groups(m, r["S"], "encoder"), worst)
    assert n == m.n_layers * m.encoder_layers * (2 * r["case"]["B"] + 1)
    _report("encoder %s" % name, worst)


# ------------------------------------------------------------------------------------------------ wiring audit
@pytest.mark.parametrize("name", DEC_CASES)
def test_decoder_every_operand_is_what_the_reference_says(tiny_cfg, name):
    r = run_decoder(tiny_cfg, name)
    _restore(r["model"], r["grads"])
    placed = cpt.audit_decoder(r["tape"].since("backward"), r["model"], r["S"], r["dset"], r["d_eps"], r["case"]["keep"])
    print("compressor-tape decoder %-8s wiring: %d calls placed, every link and every final .grad bit-equal" % (name, placed))


@pytest.mark.parametrize("name", DEC_CASES)
def test_topdown_every_operand_is_what_the_reference_says(tiny_cfg, name):
    r = run_topdown(tiny_cfg, name)
    _restore(r["model"], r["grads"])
    placed = cpt.audit_topdown(r["tape"].since("backward"), r["model"], r["S"], r["dset"], r["kl_scale"], r["d_eps"], r["d_enc"], r["case"]["keep"])
    print("compressor-tape top-down %-8s wiring: %d calls placed, every link and every final .grad bit-equal" % (name, placed))


@pytest.mark.parametrize("name", ENC_CASES)
def test_encoder_every_operand_is_what_the_reference_says(tiny_cfg, name):
    r = run_encoder(tiny_cfg, name)
    _restore(r["model"], r["grads"])
    placed = cpt.audit_encoder(r["tape"].since("backward"), r["model"], r["S"], r["d_enc"], r["d_tokens"], r["d_pos"])
    print("compressor-tape encoder %-14s wiring: %d calls placed, every link and every final .grad bit-equal" % (name, placed))


def test_chain_topdown_then_encoder_on_one_tape(tiny_cfg):
    """TopDownTrainStep on EncoderTrainStep's outputs, then EncoderTrainStep.backward on the d_enc_out it returned: both tables on one
    tape, and each d_enc_out[i] the encoder reads bit-equal to what the top-down step left."""
    r = run_topdown(tiny_cfg, "ragged", then_encoder=True)
    m, tape = r["model"], r["tape"]
    top = tape.calls[tape.marks["backward"]:r["n_backward"]]
    enc = tape.since("encoder backward")
    worst = cpt.audit_numeric(top + enc)
    cpt.audit_centred(tape.calls[tape.marks["encoder forward"]:tape.marks["forward"]], cpt.centred_groups(m, r["enc_S"], "encoder"), worst)
    cpt.audit_centred(tape.calls[tape.marks["forward"]:tape.marks["backward"]], cpt.centred_groups(m, r["S"], "topdown"), worst)
    _report("chain ragged", worst)
    _restore(m, r["grads"])
    _restore(m, r["enc_grads"])
    a = cpt.audit_topdown(top, m, r["S"], r["dset"], r["kl_scale"], r["d_eps"], r["d_enc"], r["case"]["keep"])
    b = cpt.audit_encoder(enc, m, r["enc_S"], r["d_enc"], r["d_tokens"], r["d_pos"])
    print("compressor-tape chain ragged wiring: %d + %d calls placed" % (a, b))


# ------------------------------------------------------------------------------------------------ the yardstick
def _cpu(d):
    return {k: v.detach().cpu() for k, v in d.items()}


@pytest.mark.parametrize("name", DEC_CASES)
def test_decoder_against_the_float64_oracle_at_the_twin_yardstick(tiny_cfg, name):
    from test_gpu_decoder_train import check_against_twin, oracle_step
    r = run_decoder(tiny_cfg, name)
    c = r["case"]
    names = list(r["grads"])
    args = (c["init"], c["cfg"], names, c["eps"], c["target"])
    ref = oracle_step(*args, torch.float64, keep_mask=c["keep"], d_set=c["d_set"])[0]
    twin = oracle_step(*args, torch.float32, keep_mask=c["keep"], autocast=True, d_set=c["d_set"])[0]
    got = _cpu(r["grads"])
    got["d_eps"] = r["d_eps"].cpu()
    check_against_twin(got, ref, twin, "compressor-tape decoder %s" % name)


@pytest.mark.parametrize("name", DEC_CASES)
def test_topdown_against_the_float64_restatement_at_the_twin_yardstick(tiny_cfg, name):
    import topdown_train_checks as tc
    from test_gpu_decoder_train import check_against_twin
    r = run_topdown(tiny_cfg, name)
    c = r["case"]
    names = list(r["grads"])
    args = (c["init"], c["cfg"], names, c["enc_out"], c["post_noise"], c["target"])
    ref = tc.oracle_step(*args, torch.float64, cpt.KL_WEIGHT, keep_mask=c["keep"], d_set=c["d_set"])[0]
    twin = tc.oracle_step(*args, torch.float32, cpt.KL_WEIGHT, keep_mask=c["keep"], autocast=True, d_set=c["d_set"])[0]
    got = _cpu(r["grads"])
    got.update({"d_enc_out.%d" % i: t.cpu() for i, t in enumerate(r["d_enc"])})
    check_against_twin(got, ref, twin, "compressor-tape top-down %s" % name)


@pytest.mark.parametrize("name", ENC_CASES)
def test_encoder_against_the_float64_restatement_at_the_twin_yardstick(tiny_cfg, name):
    import encoder_train_checks as ec
    from test_gpu_decoder_train import check_against_twin
    r = run_encoder(tiny_cfg, name)
    c = r["case"]
    names = list(r["grads"])
    args = (c["init"], c["cfg"], names, c["tokens"], c["pos"], c["d_enc"])
    ref = ec.encoder_step(*args, torch.float64)[0]
    twin = ec.encoder_step(*args, torch.float32, autocast=True)[0]
    got = _cpu(r["grads"])
    got["d_tokens"], got["d_pos"] = r["d_tokens"].cpu(), r["d_pos"].cpu()
    check_against_twin(got, ref, twin, "compressor-tape encoder %s" % name)


# ------------------------------------------------------------------------------------------------ exact structure probes (zeros need no bound)
def _only_sample_1(t):
    t = t.clone()
    t[0].zero_()
    t[2:].zero_()
    return t


def _isolated(r, rows, B, skip=()):
    """Every recorded output of the backward with one row per token / point / sample: exactly 0 outside sample 1, non-zero inside."""
    seen = 0
    for call in r["tape"].since("backward"):
        outs = [(k, d["after"].value) for k, d in call.inplace.items()] + [("output %d" % i, o.value) for i, o in enumerate(call.outs) if o is not None]
        for k, v in outs:
            if (call.name, k) in skip or not v.is_floating_point() or v.dim() != 2:
                continue
            per_sample = k in ("dshift", "dscale", "dgate") and v.shape[0] == B
            if v.shape[0] in rows or per_sample:
                n = 1 if per_sample else v.shape[0] // B
                inside = torch.zeros(v.shape[0], dtype=torch.bool, device=v.device)
                inside[n:2 * n] = True
                assert float(v[~inside].abs().max()) == 0.0 and float(v[inside].abs().max()) > 0.0, "%s: %s" % (call, k)
                seen += 1
    return seen


def test_topdown_a_gradient_in_one_sample_stays_in_that_sample(tiny_cfg):
    """d_set zero outside sample 1 and kl_scale 0 (the KL term reaches every sample): every per-row recorded gradient of sample 0 — dX, dkv,
    dq, dpost, the d_eps rows — is exactly 0, and so are its d_enc_out rows; sample 1's are not."""
    c = cpt.CASES["ragged"]
    B, N, T = c["B"], c["N"], c["T"]
    r = run_topdown(tiny_cfg, "ragged", edit=_only_sample_1, key="ragged/sample 1", kl_scale=0.0)
    seen = _isolated(r, (B * N, B * T), B, skip={("silu_bwd", "output 1")})      # (SiLU(x3) is no gradient)
    assert seen >= 30 * c["levels"]
    for t in r["d_enc"] + [r["d_eps"]]:
        assert float(t[0].abs().max()) == 0.0 and float(t[1].abs().max()) > 0.0


def test_encoder_a_gradient_in_one_sample_stays_in_that_sample(tiny_cfg):
    """d_enc_out zero outside sample 1 of the `odd` encoder case (B = 3): every dmod row and every per-token gradient of samples 0 and 2 is
    exactly 0, d_tokens and d_pos included."""
    c = cpt.CASES["odd-enc"]
    B, T, L, E = c["B"], c["T"], c["levels"], c["enc_layers"]
    r = run_encoder(tiny_cfg, "odd-enc", edit=_only_sample_1, key="odd-enc/sample 1")
    seen = _isolated(r, (B * T,), B)
    assert seen >= L * (2 + 6 * E) + 10 * L * E
    for t in (r["d_tokens"], r["d_pos"]):
        assert float(t[[0, 2]].abs().max()) == 0.0 and float(t[1].abs().max()) > 0.0


@pytest.mark.parametrize("step", ["decoder", "topdown"])
def test_a_prior_row_no_sample_keeps_gets_an_exactly_zero_gradient(tiny_cfg, step):
    r = (run_decoder if step == "decoder" else run_topdown)(tiny_cfg, "ragged")
    held = r["case"]["keep"].sum(0)
    g = r["grads"]["init_set.prior"].cpu()
    assert int((held == 0).sum()) >= 1 and bool((g[held == 0] == 0).all()) and bool((g[held > 0].abs().amax(1) > 0).all())


def test_a_second_forward_and_backward_gives_the_same_bits(tiny_cfg):
    a, b = run_decoder(tiny_cfg, "ragged"), run_decoder(tiny_cfg, "ragged", key="ragged/again")
    assert torch.equal(a["pts"], b["pts"]) and torch.equal(a["d_eps"], b["d_eps"]) and all(torch.equal(a["grads"][n], b["grads"][n]) for n in a["grads"])
    a, b = run_topdown(tiny_cfg, "ragged"), run_topdown(tiny_cfg, "ragged", key="ragged/again")
    assert torch.equal(a["pts"], b["pts"]) and torch.equal(a["d_eps"], b["d_eps"]) and all(torch.equal(x, y) for x, y in zip(a["d_enc"], b["d_enc"]))
    assert all(torch.equal(a["grads"][n], b["grads"][n]) for n in a["grads"])
    a, b = run_encoder(tiny_cfg, "ragged"), run_encoder(tiny_cfg, "ragged", key="ragged/again")
    assert all(torch.equal(x, y) for x, y in zip(a["outs"], b["outs"])) and torch.equal(a["d_tokens"], b["d_tokens"]) and torch.equal(a["d_pos"], b["d_pos"])
    assert all(torch.equal(a["grads"][n], b["grads"][n]) for n in a["grads"])
