"""CPU (no GPU needed): the references, bounds and planted faults of the top-down training kernels (tests/topdown_train_checks.py), and the
argument errors of the two entry points (ldt_attention_bwd_wide: csrc/attention_bwd.hip; ldt_reparam_kl_bwd: csrc/eval_loss.hip).

  * the binding's signatures against the header: the wide entry takes ldt_attention_bwd_cross's parameters + scratch and its length
  * the fp32 emulation of the chunked row statistics and dQ sits inside the float64 reference's bound, and each planted fault leaves it:
    a chunk's partial dropped from dq, chunk sums combined without exp(m_c - M), partials added unscaled; the same with a whole chunk
    whose exp(m_c - M) underflows
  * the closed form of ldt_reparam_kl_bwd equals float64 autograd over the reference's expressions, with logvar below lo, above hi and
    exactly on both bounds; its fp32 evaluation sits inside the bound and each planted fault leaves it: clamp mask ignored, -kl_scale / 2
    dropped, KL term on d_eps dropped
  * every refusal of the entry points and of the wrappers comes back with its message: no launch

Before the two entry points existed every test here ended at the missing symbol, wrapper or helper module."""
import inspect
import re

import pytest
import torch

import kernel_checks as kc
import narrow_bwd_checks as nb
import topdown_train_checks as tc


def fails(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib
    return _lib


def test_signatures_agree_with_the_header(built):
    _lib = built
    src = open(_lib._HERE + "/../include/ldt_hip.h").read()
    assert "#define LDT_ATTN_BWD_WIDE_MAX_KEYS 8192" in src and "#define LDT_ATTN_BWD_WIDE_CHUNK 256" in src
    assert (_lib.ATTN_BWD_WIDE_MAX_QUERIES, _lib.ATTN_BWD_WIDE_MAX_KEYS, _lib.ATTN_BWD_WIDE_CHUNK) == (512, 8192, 256) and tc.CHUNK == 256
    assert _lib.ABI_VERSION == 26 and _lib.lib().ldt_abi_version() == 26
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    params = lambda name: [p.strip() for p in re.search(r"\bint %s\s*\(([^)]*)\)" % name, decl).group(1).split(",")]
    cross, wide = params("ldt_attention_bwd_cross"), params("ldt_attention_bwd_wide")
    assert wide == cross[:-1] + ["float* scratch", "int64_t scratch_len", "void* stream"]                  # cross's parameters + 2
    assert len(_lib.SIGNATURES["ldt_attention_bwd_wide"]) == len(wide) == len(_lib.SIGNATURES["ldt_attention_bwd_cross"]) + 2
    assert _lib.SIGNATURES["ldt_attention_bwd_wide"] == _lib.SIGNATURES["ldt_attention_bwd_long"]
    rk = params("ldt_reparam_kl_bwd")
    assert [p.split()[-1] for p in rk] == ["post", "noise", "d_eps", "ldd", "kl_scale", "dpost", "rows", "z", "lo", "hi", "stream"]
    assert len(_lib.SIGNATURES["ldt_reparam_kl_bwd"]) == len(rk)
    import ctypes
    kinds = {"float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    assert _lib.SIGNATURES["ldt_reparam_kl_bwd"] == [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in rk]


@pytest.mark.parametrize("B,H,Nq,Nk", [(2, 2, 32, 296), (1, 4, 72, 552)])
def test_wide_attention_backward_emulation_and_planted_faults(B, H, Nq, Nk):
    q, kv, do = tc.wide_case(B, H, Nq, Nk)
    o = nb.forward_o(q, kv, B, H, Nq, Nk, 32)
    got, L = tc.wide_emulate(q, kv, o, do, B, H, Nq, Nk)
    r = tc.wide_check(got, q, kv, o, do, B, H, Nq, Nk, "fp32 emulation")
    assert max(r.values()) < 1.0
    L64 = torch.logsumexp(nb.scores64(q, kv, B, H, Nq, Nk, 32), -1, keepdim=True)
    chunks = -(-Nk // tc.CHUNK)
    assert float((L.double() - L64).abs().max()) <= (chunks + 3) * kc.U24 + kc.LIBM_ABS + 8 * kc.U24 * float(L64.abs().max() + 8)
    tc.wide_check(nb.emulate(q, kv, o, do, B, H, Nq, Nk, 32, True), q, kv, o, do, B, H, Nq, Nk, "unchunked emulation")
    for fault in tc.WIDE_FAULTS:
        fails(tc.wide_check, tc.wide_emulate(q, kv, o, do, B, H, Nq, Nk, fault=fault)[0], q, kv, o, do, B, H, Nq, Nk, fault)
    ref1, tol1 = tc.wide_ref(q, kv, o, do, B, H, Nq, Nk, chunk=8192)     # the extra terms are present exactly when there is more than one chunk
    ref2, tol2 = tc.wide_ref(q, kv, o, do, B, H, Nq, Nk)
    for nm in ("dq", "dk", "dv"):
        assert torch.equal(ref1[nm], ref2[nm]) and bool((tol2[nm] >= tol1[nm]).all()) and bool((tol2[nm] > tol1[nm]).any())
        assert float((tol2[nm] / tol1[nm]).max()) < 1.05                 # and they are small against the bf16 terms
    _, tol0 = kc.attn_bwd_ref(q, kv[:, :H * 32], kv[:, H * 32:], o, do, B, H, Nq, Nk, 32, True)
    assert all(torch.equal(tol0[nm], tol1[nm]) for nm in tol0)           # one chunk: attn_bwd_ref's bound as it stands


def test_wide_attention_one_chunk_emulation_has_the_unchunked_bits():
    B, H, Nq, Nk = 1, 2, 8, 16
    q, kv, do = tc.wide_case(B, H, Nq, Nk)
    o = nb.forward_o(q, kv, B, H, Nq, Nk, 32)
    got, _ = tc.wide_emulate(q, kv, o, do, B, H, Nq, Nk)
    whole = nb.emulate(q, kv, o, do, B, H, Nq, Nk, 32, True)
    tc.wide_check(got, q, kv, o, do, B, H, Nq, Nk, "one chunk")
    assert torch.equal(got["dq"], whole["dq"])                           # exp(0) = 1, and one partial times the scale rounds as the direct product does


def test_wide_attention_with_an_underflowing_chunk():
    B, H, Nq, Nk = tc.UNDERFLOW_SHAPE
    q, kv, do, margin = tc.underflow_case()
    assert margin >= 40.0, margin
    o = nb.forward_o(q, kv, B, H, Nq, Nk, 32)
    got, L = tc.wide_emulate(q, kv, o, do, B, H, Nq, Nk)
    assert bool(L.isfinite().all())
    tc.wide_check(got, q, kv, o, do, B, H, Nq, Nk, "fp32 emulation, chunk 0 underflows")
    fails(tc.wide_check, tc.wide_emulate(q, kv, o, do, B, H, Nq, Nk, fault="chunk sums combined without exp(m_c - M)")[0], q, kv, o, do, B, H, Nq, Nk, "")


@pytest.mark.parametrize("rows,z", tc.RKB_SHAPES)
@pytest.mark.parametrize("kl_scale", [0.0, 0.046875])               # exact in fp32, as the entry point takes it
def test_reparam_kl_bwd_closed_form_equals_autograd(rows, z, kl_scale):
    lo, hi = -6.0, 10.0
    post, noise, d_eps = tc.rkb_case(rows, z, lo, hi)
    raw = post[:, z:]
    assert bool((raw < lo).any()) and bool((raw > hi).any()) and bool((raw == lo).any()) and bool((raw == hi).any())
    want = tc.reparam_kl_bwd_autograd(post, noise, d_eps, kl_scale, lo, hi)
    ref, tol = tc.reparam_kl_bwd_closed(post, noise, d_eps, kl_scale, lo, hi)
    assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())
    out = (raw < lo) | (raw > hi)
    assert bool((ref[:, z:][out] == 0).all()) and bool((want[:, z:][out] == 0).all()) and bool((tol[:, z:][out] == 0).all())
    on = (raw == lo) | (raw == hi)
    if kl_scale:
        assert bool((want[:, z:][on] != 0).all())                        # torch's clamp passes the gradient on the bounds themselves
    assert float((tol / ref.abs().clamp_min(1e-30))[ref != 0].median()) < 1e-5        # a bound of a few fp32 roundings, not a loose one


@pytest.mark.parametrize("rows,z", tc.RKB_SHAPES)
def test_reparam_kl_bwd_emulation_and_planted_faults(rows, z):
    lo, hi, ks = -6.0, 10.0, 0.05
    post, noise, d_eps = tc.rkb_case(rows, z, lo, hi)
    ref, tol = tc.reparam_kl_bwd_closed(post, noise, d_eps, ks, lo, hi)
    r = kc.assert_elementwise(tc.reparam_kl_bwd_closed(post, noise, d_eps, ks, lo, hi, dt=torch.float32), ref, tol, "fp32 evaluation")
    assert r < 1.0
    for fault in tc.RKB_FAULTS:
        fails(kc.assert_elementwise, tc.reparam_kl_bwd_closed(post, noise, d_eps, ks, lo, hi, dt=torch.float32, fault=fault), ref, tol, fault)


def test_wrappers_have_no_fallback_and_check_their_arguments():
    from ldt_amd import ops
    from ldt_amd._lib import LdtHipError
    assert list(inspect.signature(ops.attention_bwd_wide).parameters) == list(inspect.signature(ops.attention_bwd_long).parameters)
    assert ops.attention_bwd_wide_scratch(16, 4, 32, 2048) == 8 * 16 * 4 * 32 * 34 and ops.attention_bwd_wide_scratch(1, 1, 1, 256) == 34
    assert ops.attention_bwd_wide_scratch(1, 1, 1, 257) == 68
    assert list(inspect.signature(ops.reparam_kl_bwd).parameters) == ["post", "noise", "d_eps", "kl_scale", "lo", "hi"]
    with pytest.raises(LdtHipError, match="no CPU fallback"):
        ops.reparam_kl_bwd(torch.zeros(4, 8), torch.zeros(4, 4), torch.zeros(4, 4), 0.1, -6.0, 10.0)
    z = torch.zeros(8, 64, dtype=torch.bfloat16)
    with pytest.raises(LdtHipError, match="no CPU fallback"):
        ops.attention_bwd_wide(z, z, z, torch.zeros(1, 2, 8, 32, dtype=torch.bfloat16), torch.zeros(1, 2, 8, 32, dtype=torch.bfloat16), 1, 2, 8, 8,
                               scratch=torch.zeros(8))


def test_entry_points_return_argument_errors(built):
    """Null pointers, shapes, strides and the scratch length come back as status codes with a message: no launch, so no GPU needed."""
    lib = built.lib()
    args = [16, 128, 1024, 16, 128, 16, 128, 1024, 16, 16, 16, 16, 128, 1024, 16, 128, 16, 128, 1024]
    f = lib.ldt_attention_bwd_wide
    big = 1 << 40
    assert f(*([None] + args[1:]), 1, 2, 8, 8, 32, 16, big, None) == -1 and b"null" in lib.ldt_last_error()
    assert f(*args, 1, 2, 8, 8, 32, None, big, None) == -1 and b"attention_bwd_wide: null pointer" in lib.ldt_last_error()
    for dh in (64, 16, 8, 0):
        assert f(*args, 1, 2, 8, 8, dh, 16, big, None) == -2 and b"head_dim %d (32 only)" % dh in lib.ldt_last_error()
    assert f(*args, 1, 2, 8, 8200, 32, 16, big, None) == -2 and b"Nq 8, Nk 8200 (1 <= Nq <= 512, 1 <= Nk <= 8192)" in lib.ldt_last_error()
    assert f(*args, 1, 2, 520, 8, 32, 16, big, None) == -2 and b"Nq 520" in lib.ldt_last_error()
    assert f(*args, 1, 2, 0, 8, 32, 16, big, None) == -2 and f(*args, 1, 2, 8, 0, 32, 16, big, None) == -2
    need = 2 * 1 * 2 * 8 * 34                                            # two chunks of keys
    assert f(*args, 1, 2, 8, 300, 32, 16, need - 1, None) == -1 and b"scratch holds %d floats" % (need - 1) in lib.ldt_last_error()
    assert f(*args, 0, 2, 8, 8, 32, 16, big, None) in (-1, -2)
    assert f(*(args[:1] + [132] + args[2:]), 1, 2, 8, 8, 32, 16, big, None) == -3
    assert f(*(args[:1] + [32] + args[2:]), 1, 2, 8, 8, 32, 16, big, None) == -2 and b"shorter than heads" in lib.ldt_last_error()
    # the entry points that were there keep their limits
    assert lib.ldt_attention_bwd_cross(*args, 1, 2, 8, 520, 32, None) == -2 and b"Nk 520" in lib.ldt_last_error()
    assert lib.ldt_attention_bwd_long(*args, 1, 2, 8, 520, 32, 16, big, None) == -2
    g = lib.ldt_reparam_kl_bwd
    assert g(None, 16, 16, 8, 0.1, 16, 4, 8, -6.0, 10.0, None) == -1 and b"reparam_kl_bwd: null pointer" in lib.ldt_last_error()
    assert g(16, 16, 16, 8, 0.1, None, 4, 8, -6.0, 10.0, None) == -1
    assert g(16, 16, 16, 8, 0.1, 16, 0, 8, -6.0, 10.0, None) == -2 and g(16, 16, 16, 8, 0.1, 16, 4, 0, -6.0, 10.0, None) == -2
    assert g(16, 16, 16, 7, 0.1, 16, 4, 8, -6.0, 10.0, None) == -2 and b"ldd 7" in lib.ldt_last_error()


# ------------------------------------------------------------------------------------------------ the step and the trainer, on the CPU
def _compressor(tiny_cfg, **kw):
    import copy
    import ldt_amd
    c = copy.deepcopy(tiny_cfg.compressor)
    for k, v in kw.items():
        setattr(c, k, v)
    return ldt_amd.Compressor(c)


def test_refuse_untrainable_topdown_names_each_reason(tiny_cfg):
    from ldt_amd.compressor_train import DecoderTrainStep, TopDownTrainStep, refuse_untrainable_topdown
    refuse_untrainable_topdown(_compressor(tiny_cfg))                    # the tiny config itself is covered; parameters on the CPU
    for kw, msg in ((dict(class_condition=True, num_categorys=3), "class_condition"),
                    (dict(decoder_act="relu"), "decoder_act='relu'"),
                    (dict(norm="group_norm"), "norm='group_norm'.*layer_norm"),
                    (dict(max_outputs=None), "max_outputs: None.*mixture"),
                    (dict(decoder_dropout_p=0.1), "decoder_dropout_p=0.1"),
                    (dict(num_heads=4), "32-wide attention heads.*hidden 64 / 4 heads"),
                    (dict(z_scales=520), "top-down half with 520 latent tokens on 64 set points.*ldt_attention_bwd_wide takes 1 <= Nq <= 512, 1 <= Nk <= 8192")):
        with pytest.raises(NotImplementedError, match=msg):
            TopDownTrainStep(_compressor(tiny_cfg, **kw))
    m = _compressor(tiny_cfg)
    with pytest.raises(NotImplementedError, match="top-down half with 8 latent tokens on 8200 set points.*1 <= Nk <= 8192"):
        refuse_untrainable_topdown(m, num_points=8200)
    with pytest.raises(ValueError, match="100 set points from 64 prior rows"):
        refuse_untrainable_topdown(m, num_points=100)
    assert (TopDownTrainStep.MAX_TOKENS, TopDownTrainStep.MAX_POINTS) == (512, 8192)
    step = TopDownTrainStep(m)
    enc = [torch.zeros(2, 8, 64)] * 3
    nz = [torch.zeros(2, 8, 40)] * 3
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        step.forward(enc, nz)
    with pytest.raises(RuntimeError, match="before forward"):
        step.backward(torch.zeros(2, 64, 3), 0.1)
    assert list(inspect.signature(TopDownTrainStep.forward).parameters) == ["self", "enc_out", "post_noise", "num_points", "keep_mask"]
    assert list(inspect.signature(TopDownTrainStep.backward).parameters) == ["self", "dset", "kl_scale"]
    # the decoder step keeps its interface and its messages
    assert list(inspect.signature(DecoderTrainStep.forward).parameters) == ["self", "eps", "num_points", "keep_mask"]
    with pytest.raises(NotImplementedError, match="64 set points on 520 latent tokens.*1 <= Nk <= 512"):
        DecoderTrainStep(_compressor(tiny_cfg, z_scales=520))


def test_topdown_parameters_are_the_top_down_half(tiny_cfg):
    from ldt_amd.compressor_train import decoder_parameters, topdown_parameters
    m = _compressor(tiny_cfg)
    names = [n for n, _ in topdown_parameters(m)]
    every = [n for n, _ in m.named_parameters()]
    assert names == [n for n in every if n in set(names)]                # module order
    dec = [n for n, _ in decoder_parameters(m)]
    assert set(dec) < set(names) and [n for n in names if n in set(dec)] == dec
    for l in range(3):
        for leaf in ("att.fc_q.weight", "att.fc_kv.bias", "att.fc_o.weight", "att.norm1.norm.weight", "att.norm2.norm.bias",
                     "att.mlp.fc.0.0.weight", "att.mlp.out.bias", "prior.1.weight", "prior.1.bias"):
            assert "decoder.%d.%s" % (l, leaf) in names
    rest = [n for n in every if n not in names]
    assert rest and all(n.startswith(("input.", "conv_in.", "encoder.", "group.", "pos_embedding.")) for n in rest), rest
    assert len(names) == len(dec) + 3 * (14 + 2)


def test_update_topdown_on_the_cpu_has_no_fallback_and_allocates_nothing(tiny_cfg):
    import copy
    import ldt_amd
    tr = ldt_amd.CompressorTrainer(tiny_cfg, ldt_amd.Compressor(tiny_cfg.compressor), "cpu")
    assert tr.kl_weight is None and tr.topdown_optimizer is None and tr.last_enc_out_grad is None
    with pytest.raises(ValueError, match="kl_weight is not set"):
        tr.update_topdown({"tr_points": torch.zeros(2, 64, 3)})
    cfg = copy.deepcopy(tiny_cfg)
    cfg.opt.kl_weight = 0.5
    tr = ldt_amd.CompressorTrainer(cfg, ldt_amd.Compressor(cfg.compressor), "cpu")
    with pytest.raises(RuntimeError, match="update_topdown: device cpu; the HIP path has no CPU fallback"):
        tr.update_topdown({"tr_points": torch.zeros(2, 64, 3)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.update_topdown({"tr_points": torch.zeros(2, 64, 3)}, enc_out=[torch.zeros(2, 8, 64)] * 3, post_noise=[torch.zeros(2, 8, 40)] * 3)
    assert tr.topdown_optimizer is None and tr.optimizer is None and tr.itr == 0 and all(p.grad is None for p in tr.model.parameters())
    ct = ldt_amd.CompletionCompressorTrainer(cfg, ldt_amd.Compressor(cfg.compressor), "cpu")
    with pytest.raises(NotImplementedError, match="CompletionCompressorTrainer.update_topdown.*CompressorTrainer alone"):
        ct.update_topdown({"tr_points": torch.zeros(2, 64, 3)})
    assert ct.topdown_optimizer is None
    with pytest.raises(NotImplementedError, match="CompressorTrainer.update: training \\(optimizer step, backward\\) is not on this path"):
        tr.update({})                                                    # update and compute_loss keep refusing, with their messages
    with pytest.raises(NotImplementedError, match="CompressorTrainer.compute_loss: its EMD_loss term"):
        tr.compute_loss(None, None)
    kw = [p.name for p in inspect.signature(ldt_amd.CompressorTrainer.update_topdown).parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert kw == ["enc_out", "post_noise"]
    bad = ldt_amd.CompressorTrainer(cfg, _compressor(cfg, decoder_act="relu"), "cpu")
    with pytest.raises(NotImplementedError, match="decoder_act"):
        bad.update_topdown({"tr_points": torch.zeros(2, 64, 3)})
    with pytest.raises(RuntimeError, match="Compressor.bottom_up: parameters on cpu"):
        tr.model.bottom_up(torch.zeros(2, 64, 3))
    assert list(inspect.signature(ldt_amd.Compressor.bottom_up).parameters) == ["self", "x", "label"]
