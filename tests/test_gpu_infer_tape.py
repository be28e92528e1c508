"""GPU (-m gpu): `Compressor.forward` and `Compressor.sample` audited call by call (tests/infer_tape.py; its teeth are shown on the CPU by
test_infer_tape_host.py).

The stand-alone kernel tests hold every kernel alone on operands the test built, and the goldens hold a whole forward at 1e-4.  Inside a
forward the kernels run on operands neither gives them: column views of the modulation rows addressed by a sample stride, the two halves of
one K | V buffer, a token stream and a set stream updated in place by two kinds of call per block, a bf16 image written by another kernel's
store pass and read a level later, the column slice all_eps[:, z j : z (j + 1)] as a draw's destination and the next GEMM's operand, a query
projection handed from one level's last kernel to the next level's first.  Here each forward runs with the `ops` of ldt_amd.compressor and
ldt_amd.blocks replaced by a recording proxy, and
  * every recorded call (the packing's included) is held per element against float64 from ITS OWN recorded operands with the bound that
    holds the kernel alone (err / bound <= 1), the storage around every destination unchanged;
  * every operand is bit-equal to what the reference says it must be (audit_forward / audit_sample), no call is left unplaced, and the
    returned tensors are what the named calls left;
  * the taped run returns the bits of an untaped one;
  * the cases together reach every entry point the two modules can.
Each run is made once per module and shared.  The worst err / bound per call kind is printed (-s); DESIGN.md section 4.20 records them."""
import pytest
import torch

import infer_tape as it
import train_tape as tt

pytestmark = pytest.mark.gpu

_RUNS, WORST = {}, {}
# (case, mode, want_kl, a subset of the prior rows kept)
RUNS = [("fused", "forward", False, False), ("fused", "forward", True, True), ("chain", "forward", False, False), ("grouped", "forward", True, False),
        ("fused", "sample", False, True), ("chain", "sample", False, False)]
_id = lambda r: "%s-%s%s%s" % (r[0], r[1], "-kl" if r[2] else "", "-dropped" if r[3] else "")


@pytest.fixture(scope="module", autouse=True)
def _release_the_tapes():
    yield
    _RUNS.clear()


def _forward(model, r, B, npts):
    torch.manual_seed(4)
    if r["mode"] == "forward":
        return model(r["x"], num_points=npts, post_noise=r["post_noise"], want_kl=r["want_kl"], want_stats=r["want_kl"])
    return model.sample((B, npts), given_eps=r["eps"], keep_mask=r["keep"], seed_eps=r.get("seed_eps"))


def run(tiny_cfg, key):
    if key in _RUNS:
        return _RUNS[key]
    import ldt_amd.compressor as cm
    which, mode, want_kl, dropped = key
    over, B, N = it.CASES[which]
    model, _ = it.make_case(tiny_cfg.compressor, **over)
    model = model.cuda()
    tape = tt.Tape(cm.ops)
    T, z, Ld = model.z_scales, model.z_dim, model.n_layers
    g = torch.Generator().manual_seed(9)
    npts = it.DROPPED if dropped else model.outsize
    r = dict(model=model, tape=tape, mode=mode, B=B, want_kl=want_kl, npts=npts, keep=None, post_noise=None)
    if mode == "forward":
        r["x"] = it.clouds(B, N, 3).cuda()
        if which != "chain":                                                # the chain case lets the forward draw on the device
            r["post_noise"] = [torch.randn(B, T, z, generator=g).cuda() for _ in range(Ld)]
    else:
        r["eps"] = torch.randn(B, T, Ld * z, generator=g).cuda()
        if dropped:
            r["keep"] = torch.stack([torch.randperm(model.max_outputs, generator=g) < npts for _ in range(B)])
        if model.max_outputs is None:
            r["seed_eps"] = torch.randn(B, npts, model.init_set.n_mixtures, model.hidden_dim, generator=g).cuda()
    with pytest.MonkeyPatch.context() as mp:
        tt.install_infer_ops(mp, tape)
        model.packed()
        tape.mark("forward")
        r["res"] = _forward(model, r, B, npts)
    torch.cuda.synchronize()
    if mode == "forward" and dropped:                                       # the rows the forward drew first (Network.py:215 before :220)
        torch.manual_seed(4)
        r["keep"] = model._presence(B, npts)
    _RUNS[key] = r
    return r


@pytest.mark.parametrize("key", RUNS, ids=_id)
def test_every_call_within_the_bound_of_its_kernel(tiny_cfg, key):
    r = run(tiny_cfg, key)
    worst = it.audit_numeric(r["tape"].calls, it.grouper_ctx(r["model"]))
    for k in sorted(worst):
        print("%-22s %-64s %.4f" % (_id(key), k, worst[k]))
        WORST[k] = max(WORST.get(k, 0.0), worst[k])
    bad = {k: v for k, v in it.ratios(worst).items() if not v <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("key", RUNS, ids=_id)
def test_every_operand_is_what_the_reference_says(tiny_cfg, key):
    r = run(tiny_cfg, key)
    calls = r["tape"].since("forward")
    if r["mode"] == "forward":
        n = it.audit_forward(calls, r["model"], r["x"], r["res"], post_noise=r["post_noise"], keep_mask=r["keep"], want_kl=r["want_kl"], num_points=r["npts"])
    else:
        n = it.audit_sample(calls, r["model"], r["B"], r["npts"], r["eps"], r["res"], keep_mask=r["keep"], seed_eps=r.get("seed_eps"))
    assert n == len(calls)


@pytest.mark.parametrize("key", [k for k in RUNS if k[0] != "chain" or k[1] == "sample"], ids=_id)
def test_the_taped_run_returns_the_bits_of_an_untaped_one(tiny_cfg, key):
    """(The chain forward draws its noise from one CPU draw: seeded alike, and every kernel being deterministic, it would pass too; it is left
    to the two audits.)"""
    r = run(tiny_cfg, key)
    again = _forward(r["model"], r, r["B"], r["npts"])
    if r["mode"] == "sample":
        assert torch.equal(again, r["res"])
    else:
        assert torch.equal(again["set"], r["res"]["set"]) and torch.equal(again["all_eps"], r["res"]["all_eps"])


def test_the_cases_together_reach_every_entry_point(tiny_cfg):
    seen = set()
    for key in RUNS:
        seen |= {c.name for c in run(tiny_cfg, key)["tape"].calls}
    assert it.REACHABLE <= seen, "this case no longer reaches %s" % sorted(it.REACHABLE - seen)
    forms = {("fused", "forward", False, False): {"ln_linear", "ln_mlp_resid_", "attention_oproj_resid_", "group_normalize", "actnorm_", "reparam"},
             ("chain", "forward", False, False): {"layernorm_modulate", "attention_fwd", "mixture_seed", "norm_points", "philox_normal"},
             ("grouped", "forward", True, False): {"grouper_mlp", "group_stats", "norm_apply", "block_activation_", "reparam_kl"}}
    for key, want in forms.items():
        names = {c.name for c in run(tiny_cfg, key)["tape"].since("forward")}
        assert want <= names, "%s: this case no longer reaches %s" % (_id(key), sorted(want - names))
    r = run(tiny_cfg, RUNS[0])
    hand = [c for c in r["tape"].since("forward") if c.name == "ln_mlp_resid_" and c.args.get("next_linear") is not None]
    image = [c for c in r["tape"].since("forward") if c.name == "ln_mlp_resid_" and "x_bf16_out" in c.inplace]
    assert len(hand) == r["model"].n_layers - 1 and len(image) == r["model"].n_layers - 1, "this case no longer reaches the hand-off / the bf16 image"


def test_zz_margins():
    """Printed last (DESIGN.md section 4.20 quotes them): the worst err / bound per call kind over the runs above, then the shares."""
    for k in sorted(WORST):
        print("%-72s %.4f" % (k, WORST[k]))
    assert all(v <= 1.0 for v in it.ratios(WORST).values())
