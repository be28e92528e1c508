"""Host checks (no GPU) for Score training at head widths 8, 16 and 32: the two forms of the attention-backward bound
(kernel_checks.attn_bwd_ref), an fp32 emulation of the kernels with planted faults (tests/narrow_bwd_checks.py), the argument checks of
ldt_attention_bwd_narrow, refuse_untrainable, and the fixture tests/golden/score_train_narrow.npz against the oracle."""
import pytest
import torch

import kernel_checks as kc
import narrow_bwd_checks as nb
import train_narrow_checks as tn


@pytest.mark.parametrize("B,H,N,large", [(2, 2, 8, False), (1, 2, 72, True)])
def test_generalised_reference_is_kernel_checks_at_64(B, H, N, large):
    """The one reference (kernel_checks.attn_bwd_ref) in its two forms: only the bound differs."""
    qkv, do = nb.attn_case(B, H, N, 64, large)
    (q, kv), C = nb.split(qkv), H * 64
    o = nb.forward_o(q, kv, B, H, N, N, 64)
    ref, tol = kc.attn_bwd_ref(q, kv[:, :C], kv[:, C:], o, do, B, H, N, N, 64, rounded=True)
    ref_fp32, tol_fp32 = kc.attn_bwd_ref(q, kv[:, :C], kv[:, C:], o, do, B, H, N, N, 64, rounded=False)   # without the 2^-8 terms the bound is smaller
    assert all(torch.equal(ref_fp32[nm], ref[nm]) for nm in ("dq", "dk", "dv"))
    assert all(bool((tol_fp32[nm] <= tol[nm]).all()) and bool((tol_fp32[nm] < tol[nm]).any()) for nm in ("dq", "dk", "dv"))


def test_large_logit_cases_need_the_row_maximum():
    for B, H, N, Dh in nb.LARGE:
        s = nb.scores64(*nb.split(nb.attn_case(B, H, N, Dh, True)[0]), B, H, N, N, Dh)
        assert float(s.amax(-1).min()) > 25 and float(s.amax(-1).max()) > 89       # past fp32 exp's range


@pytest.mark.parametrize("B,H,N,Dh,large", nb.CASES)
def test_emulation_is_inside_the_bound(B, H, N, Dh, large):
    """fp32 products, fp32 L and D, bf16 outputs: inside the bound in both forms, at every shape the GPU test runs."""
    qkv, do = nb.attn_case(B, H, N, Dh, large)
    q, kv = nb.split(qkv)
    o = nb.forward_o(q, kv, B, H, N, N, Dh)
    for rounded in (True, False):
        r = nb.check(nb.emulate(q, kv, o, do, B, H, N, N, Dh, rounded), q, kv, o, do, B, H, N, N, Dh, "emulation", rounded=rounded)
        print("emulation B%d H%d N%d Dh%d large=%d rounded=%d: err / tol %.3f" % (B, H, N, Dh, large, rounded, r))
        assert r <= 1.0


@pytest.mark.parametrize("fault,B,H,N,Dh,output", [
    ("last key dropped from dq", 1, 2, 72, 8, "dq"),
    ("last query dropped from dk dv", 1, 2, 72, 16, "d[kv]"),
    ("scale 1/8", 2, 3, 8, 8, "d[qk]"),
    ("scale 1/8", 2, 4, 33, 32, "d[qk]"),
    ("D not subtracted", 2, 3, 5, 16, "d[qk]"),
    ("dO permuted", 2, 3, 8, 8, "d[qkv]"),
    ("L of the next head", 2, 3, 8, 8, "d[qkv]"),
    ("rows past N not masked", 2, 3, 5, 16, "d[qkv]"),
    ("rows past N not masked", 2, 3, 5, 8, "d[qkv]"),
])
def test_planted_faults_fail_naming_the_output(fault, B, H, N, Dh, output):
    qkv, do = nb.attn_case(B, H, N, Dh)
    q, kv = nb.split(qkv)
    o = nb.forward_o(q, kv, B, H, N, N, Dh)
    rounded = nb.rounds(Dh)
    assert nb.check(nb.emulate(q, kv, o, do, B, H, N, N, Dh, rounded), q, kv, o, do, B, H, N, N, Dh, "sound") <= 1.0
    with pytest.raises(AssertionError, match=r"planted %s: \d+ of \d+ elements outside the bound" % output):
        nb.check(nb.emulate(q, kv, o, do, B, H, N, N, Dh, rounded, fault=fault), q, kv, o, do, B, H, N, N, Dh, "planted")


def test_narrow_entry_point_returns_argument_errors():
    """Null pointers, head widths, token counts and strides come back as status codes with a message: no launch, so no GPU needed."""
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib
    lib = _lib.lib()
    assert lib.ldt_abi_version() == 26
    args = [16, 128, 1024, 16, 128, 16, 128, 1024, 16, 16, 16, 16, 128, 1024, 16, 128, 16, 128, 1024]
    f = lib.ldt_attention_bwd_narrow
    assert f(*([None] + args[1:]), 1, 2, 8, 8, None) == -1 and f(*(args[:10] + [None] + args[11:]), 1, 2, 8, 8, None) == -1
    for dh in (64, 24):
        assert f(*args, 1, 2, 8, dh, None) == -2 and b"8, 16 or 32" in lib.ldt_last_error()
    for dh in (8, 16, 32):
        assert f(*args, 1, 2, 513, dh, None) == -2 and b"N 513" in lib.ldt_last_error()
        assert f(*args, 1, 2, 0, dh, None) == -2
        assert f(*(args[:1] + [132] + args[2:]), 1, 2, 8, dh, None) == -3          # rows not 16-byte aligned
    assert f(*(args[:1] + [24] + args[2:]), 1, 4, 8, 8, None) == -2 and b"shorter than heads" in lib.ldt_last_error()   # 24 < 4 x 8
    assert f(*(args[:12] + [130] + args[13:]), 1, 2, 8, 8, None) == -3             # dQ rows not 8-byte aligned


def test_refuse_untrainable_lets_the_four_head_widths_pass(tiny_cfg):
    import copy
    import ldt_amd
    from ldt_amd.train import refuse_untrainable
    for heads in (16, 8, 4, 2):
        cfg = copy.deepcopy(tiny_cfg)
        cfg.score.num_heads = heads
        model = ldt_amd.Score(cfg.score)
        assert model.hidden_size // model.num_heads == 128 // heads
        refuse_untrainable(model)
    model.num_heads, model.hidden_size = 5, 120                                       # 24-wide heads
    with pytest.raises(NotImplementedError, match=r"8-, 16-, 32- or 64-wide attention heads .*got 24"):
        refuse_untrainable(model)


@pytest.mark.parametrize("key", list(tn.MODELS))
def test_fixture_is_tied_to_the_oracle(tiny_cfg, key):
    """The initial weights rebuilt from the seed match init_digest::*, and the fp32 oracle's iteration-0 gradients and loss match
    grad0_digest::* / loss[0] (both asserted inside), as test_gpu_train_narrow.py relies on."""
    g = tn.golden()
    grads, names, loss = tn.reference_grads0(tiny_cfg, key)
    m = tn.MODELS[key]
    assert len(names) == len(grads) and g[key + "_idx"].shape == (m["iters"], tn.B) and g[key + "_loss"].shape == (m["iters"],)
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())
    assert float(g[key + "_twin_grad_relmse_all"]) > 0 and all(key + "_twin_grad_relmse::" + n in g for n in names)
    if key == "a":
        assert float(g["a_loss"][-1]) < 0.7 * float(g["a_loss"][0]) and float(g["a_twin_loss_dev"]) > 0
    if key == "b":
        assert torch.equal(g["b_cates"], tn.CATES)
