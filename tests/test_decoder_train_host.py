"""CPU (no GPU needed): the references, bounds and planted faults of the decoder-training kernels (tests/decoder_train_checks.py), the host
index map of a keep mask, and the argument errors of the new entry points (csrc/chamfer_loss.hip, ldt_attention_bwd_long, ldt_rows_gather_sum).

  * the teacher-forced Chamfer gradient reference equals torch.autograd on a pure-torch Chamfer (explicit differences, l1 and l2), and the
    loss reference equals its loss
  * the fp32 emulation of each kernel sits inside its bound, and each planted fault leaves it: the scattered term dropped, the 1 / (B n)
    factor of the wrong direction, idx1 used for the gather, a coincident pair's NaN; a chunk's partial dropped from dK, partials added
    unscaled, a chunk reading another chunk's queries; a prior row summed over the wrong sample set
  * an index that is no argmin is caught; the lowest index of a tie and a near tie both pass
  * every refusal of the entry points comes back as a status with its message: no launch

The tests of the helper's own references and bounds (autograd, emulations, planted faults, the argmin check) need nothing of the feature
and pass without it, as reference self-tests do; the others — the index map, the wrappers, the entry points' argument errors, the step's
refusals and the trainer's surface — ended at the missing module, symbol or wrapper before it existed."""
import inspect

import pytest
import torch

import decoder_train_checks as dc
import kernel_checks as kc
import narrow_bwd_checks as nb


def fails(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


@pytest.mark.parametrize("B,n,m", dc.CD_SHAPES)
@pytest.mark.parametrize("type", ["l1", "l2"])
def test_chamfer_gradient_reference_equals_autograd(B, n, m, type):
    x1, x2 = dc.cd_case(B, n, m)
    a = x1.double().requires_grad_(True)
    loss = dc.cd_loss_torch(a, x2.double(), type)
    (want,) = torch.autograd.grad(loss * 0.75, a)
    d1, d2, i1, i2 = dc.dist_chamfer_torch(x1.double(), x2.double())
    ref, tol = dc.cd_grad(x1, x2, i1, i2, type, upstream=0.75)
    assert float((ref - want).abs().max()) <= 1e-14 * max(1.0, float(want.abs().max()))
    assert bool((tol > 0).all()) and float((tol / ref.abs().clamp_min(1e-300)).median()) < 1e-5       # a bound of a few fp32 roundings, not a loose one
    assert float((dc.cd_loss_ref(d1, d2, type)[0] - loss.detach()).abs()) <= 1e-14 * float(loss.detach())
    dc.assert_valid_argmin(x1, x2, i1, "idx1"); dc.assert_valid_argmin(x2, x1, i2, "idx2")


@pytest.mark.parametrize("type", ["l1", "l2"])
def test_chamfer_gradient_emulation_and_planted_faults(type):
    B, n, m = 2, 72, 200
    x1, x2 = dc.cd_case(B, n, m)
    x2[0, 5] = x1[0, 9]                                                  # a coincident pair: contributes exactly 0
    _, _, i1, i2 = dc.dist_chamfer_torch(x1.double(), x2.double())
    assert int(i2[0, 5]) == 9 and int(i1[0, 9]) == 5
    ref, tol = dc.cd_grad(x1, x2, i1, i2, type)
    assert bool(ref.isfinite().all())
    r = kc.assert_elementwise(dc.cd_grad(x1, x2, i1, i2, type, dt=torch.float32), ref, tol, "fp32 emulation")
    assert r < 1.0
    for fault in dc.CD_FAULTS:
        if fault == "coincident pair poisons" and type == "l2":
            continue                                                     # l2 has no root: nothing to poison
        fails(kc.assert_elementwise, dc.cd_grad(x1, x2, i1, i2, type, dt=torch.float32, fault=fault), ref, tol, fault)


def test_a_point_that_is_nobodys_nearest_gets_only_its_own_term():
    x2 = torch.tensor([[[0.0, 0, 0], [1.0, 0, 0]]])
    x1 = torch.tensor([[[0.25, 0, 0], [0.75, 0, 0], [9.0, 0, 0]]])       # the third point is far from both targets
    _, _, i1, i2 = dc.dist_chamfer_torch(x1.double(), x2.double())
    assert i2.tolist() == [[0, 1]] and i1.tolist() == [[0, 1, 1]]
    ref, _ = dc.cd_grad(x1, x2, i1, i2, "l1")
    assert ref[0, 2].tolist() == [1.0 / 3, 0.0, 0.0]                     # the unit direction over B n = 3
    ref2, _ = dc.cd_grad(x1, x2, i1, i2, "l2")
    assert abs(float(ref2[0, 2, 0]) - 2 * 8.0 / 3) < 1e-15


def test_argmin_check_catches_a_wrong_index_and_admits_ties():
    x1, x2 = dc.cd_case(1, 64, 64)
    x2[0, 40] = x2[0, 7]                                                 # a duplicated target: both indices attain the minimum
    _, _, i1, _ = dc.dist_chamfer_torch(x1.double(), x2.double())
    dc.assert_valid_argmin(x1, x2, i1, "lowest")
    alt = torch.where(i1 == 7, torch.full_like(i1, 40), i1)
    assert not torch.equal(alt, i1)
    dc.assert_valid_argmin(x1, x2, alt, "the tie's other index")
    wrong = i1.clone(); wrong[0, 3] = (int(i1[0, 3]) + 1) % 64
    fails(dc.assert_valid_argmin, x1, x2, wrong, "a neighbour that is not nearest")
    out = i1.clone(); out[0, 0] = 64
    fails(dc.assert_valid_argmin, x1, x2, out, "an index past the cloud")


@pytest.mark.parametrize("B,H,Nq,Nk", [(2, 2, 296, 32), (1, 4, 552, 72)])
def test_long_attention_backward_emulation_and_planted_faults(B, H, Nq, Nk):
    q, kv, do = dc.long_case(B, H, Nq, Nk)
    o = nb.forward_o(q, kv, B, H, Nq, Nk, 32)
    got = dc.long_emulate(q, kv, o, do, B, H, Nq, Nk)
    r = dc.long_check(got, q, kv, o, do, B, H, Nq, Nk, "fp32 emulation")
    assert max(r.values()) < 1.0
    whole = nb.emulate(q, kv, o, do, B, H, Nq, Nk, 32, True)             # one sum over all queries: the same dq bits, dk / dv inside the same bound
    assert torch.equal(whole["dq"], got["dq"])
    dc.long_check(whole, q, kv, o, do, B, H, Nq, Nk, "unchunked emulation")
    for fault in dc.LONG_FAULTS:
        fails(dc.long_check, dc.long_emulate(q, kv, o, do, B, H, Nq, Nk, fault=fault), q, kv, o, do, B, H, Nq, Nk, fault)
    ref1, tol1 = dc.long_ref(q, kv, o, do, B, H, Nq, Nk, chunk=8192)     # the partial-sum term is present exactly when there is more than one chunk
    ref2, tol2 = dc.long_ref(q, kv, o, do, B, H, Nq, Nk)
    assert torch.equal(tol1["dq"], tol2["dq"]) and bool((tol2["dk"] > tol1["dk"]).all()) and bool((tol2["dv"] >= tol1["dv"]).all())
    assert float((tol2["dk"] / tol1["dk"]).max()) < 1.01                 # and it is small against the bf16 terms


def test_prior_row_map_and_gather_sum_reference():
    from ldt_amd import ops
    keep = torch.tensor([[1, 0, 1, 1, 0], [0, 0, 1, 1, 1], [1, 1, 1, 0, 0]], dtype=torch.bool)
    src = ops.prior_row_map(keep)
    assert src.dtype == torch.int32 and src.tolist() == [[0, -1, 1, 2, -1], [-1, -1, 0, 1, 2], [0, 1, 2, -1, -1]]
    assert ops.prior_row_map(torch.ones(2, 4, dtype=torch.bool)).tolist() == [[0, 1, 2, 3]] * 2          # no mask: src[b][r] = r
    # the map restates InitialSet's own selection: prior[None].expand(B)[keep].view(B, N) puts prior row r of sample b at src[b][r]
    R, N, C = 5, 3, 4
    prior = torch.randn(R, C, dtype=torch.float64, requires_grad=True)
    x = prior[None].expand(3, -1, -1)[keep].view(3, N, C)
    dy = torch.randn(3 * N, C)
    (want,) = torch.autograd.grad((x * dy.double().view(3, N, C)).sum(), prior)
    ref, tol = dc.rows_gather_sum_ref(dy, src, N)
    assert float((ref - want).abs().max()) < 1e-14
    kc.assert_elementwise(dc.rows_gather_sum_emulate(dy, src, N), ref, tol, "fp32 emulation")
    fails(kc.assert_elementwise, dc.rows_gather_sum_emulate(dy, src, N, fault="wrong sample set"), ref, tol, "a prior row summed over the wrong samples")
    none = ops.prior_row_map(torch.tensor([[1, 0], [1, 0]], dtype=torch.bool))
    ref0, tol0 = dc.rows_gather_sum_ref(torch.randn(2, C), none, 1)
    assert bool((ref0[1] == 0).all()) and bool((tol0[1] == 0).all())     # a row nobody kept: exactly 0, and the bound leaves no room


def test_host_tensors_have_no_fallback():
    import ldt_amd.losses as losses
    from ldt_amd import ops
    from ldt_amd._lib import LdtHipError
    x1, x2 = dc.cd_case(1, 8, 8)
    with pytest.raises(LdtHipError, match="no CPU fallback"):
        losses.cd_loss(x1, x2)
    with pytest.raises(LdtHipError, match="no CPU fallback"):
        ops.rows_gather_sum(torch.zeros(8, 4), torch.zeros(1, 8, dtype=torch.int32), 8)
    with pytest.raises(ValueError, match="neither 'l1' nor 'l2'"):
        ops.cd_loss(torch.zeros(4), torch.zeros(4), "emd")
    assert list(inspect.signature(losses.cd_loss).parameters)[:4] == ["esti", "shapes", "type", "want_grad"]
    assert list(inspect.signature(ops.attention_bwd_long).parameters)[:11] == ["q", "k", "v", "o", "do", "B", "H", "Nq", "Nk", "dq_out", "dkv_out"]
    assert ops.attention_bwd_long_scratch(16, 4, 2048, 32) == 8 * 16 * 32 * 256 and ops.attention_bwd_long_scratch(1, 1, 256, 1) == 64


def test_new_entry_points_return_argument_errors():
    """Null pointers, shapes, types and the scratch length come back as status codes with a message: no launch, so no GPU needed."""
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib
    lib = _lib.lib()
    assert (_lib.ATTN_BWD_LONG_MAX_QUERIES, _lib.ATTN_BWD_LONG_MAX_KEYS, _lib.ATTN_BWD_LONG_CHUNK) == (8192, 512, 256) and _lib.CD_TYPES == {"l1": 1, "l2": 2}
    src = open(_lib._HERE + "/../include/ldt_hip.h").read()
    assert "#define LDT_ATTN_BWD_LONG_MAX_QUERIES 8192" in src and "#define LDT_ATTN_BWD_LONG_CHUNK 256" in src
    assert "#define LDT_CD_L1 1" in src and "#define LDT_CD_L2 2" in src
    f = lib.ldt_chamfer_nn
    assert f(None, 16, 1, 4, 4, 16, 16, 16, 16, None) == -1 and b"null" in lib.ldt_last_error()
    assert f(16, 16, 1, 4, 4, 16, None, 16, 16, None) == -1
    assert f(16, 16, 0, 4, 4, 16, 16, 16, 16, None) == -2 and f(16, 16, 1, 0, 4, 16, 16, 16, 16, None) == -2
    assert f(16, 16, 65536, 4, 4, 16, 16, 16, 16, None) == -2 and b"1 .. 65535" in lib.ldt_last_error()
    f = lib.ldt_cd_loss
    assert f(None, 4, 16, 4, 1, 16, None) == -1 and f(16, 0, 16, 4, 1, 16, None) == -2
    assert f(16, 4, 16, 4, 3, 16, None) == -1 and b"type 3" in lib.ldt_last_error()
    f = lib.ldt_cd_loss_bwd
    assert f(16, 16, None, 16, 1, 4, 4, 1, 1.0, 16, None) == -1 and f(16, 16, 16, 16, 1, 4, 0, 1, 1.0, 16, None) == -2
    assert f(16, 16, 16, 16, 1, 4, 4, 0, 1.0, 16, None) == -1 and b"type 0" in lib.ldt_last_error()
    f = lib.ldt_rows_gather_sum
    assert f(None, 8, 16, 1, 4, 4, 8, 16, None) == -1 and f(16, 4, 16, 1, 4, 4, 8, 16, None) == -2 and b"ld 4" in lib.ldt_last_error()
    assert f(16, 8, 16, 1, 4, 65536, 8, 16, None) == -2
    # ldt_attention_bwd_long: ldt_attention_bwd_cross's operands, then scratch and its length
    assert len(_lib.SIGNATURES["ldt_attention_bwd_long"]) == len(_lib.SIGNATURES["ldt_attention_bwd_cross"]) + 2
    args = [16, 128, 1024, 16, 128, 16, 128, 1024, 16, 16, 16, 16, 128, 1024, 16, 128, 16, 128, 1024]
    f = lib.ldt_attention_bwd_long
    big = 1 << 40
    assert f(*([None] + args[1:]), 1, 2, 8, 8, 32, 16, big, None) == -1 and b"null" in lib.ldt_last_error()
    assert f(*args, 1, 2, 8, 8, 32, None, big, None) == -1
    for dh in (64, 16, 8, 0):
        assert f(*args, 1, 2, 8, 8, dh, 16, big, None) == -2 and b"head_dim %d (32 only)" % dh in lib.ldt_last_error()
    assert f(*args, 1, 2, 8200, 8, 32, 16, big, None) == -2 and b"Nq 8200, Nk 8 (1 <= Nq <= 8192, 1 <= Nk <= 512)" in lib.ldt_last_error()
    assert f(*args, 1, 2, 8, 520, 32, 16, big, None) == -2 and b"Nk 520" in lib.ldt_last_error()
    assert f(*args, 1, 2, 0, 8, 32, 16, big, None) == -2 and f(*args, 0, 2, 8, 8, 32, 16, big, None) == -2
    assert f(*args, 1, 2, 300, 8, 32, 16, 2 * 8 * 128 - 1, None) == -2 and b"scratch holds 2047 floats" in lib.ldt_last_error()   # two chunks
    assert f(*(args[:1] + [132] + args[2:]), 1, 2, 8, 8, 32, 16, big, None) == -3
    assert f(*(args[:1] + [32] + args[2:]), 1, 2, 8, 8, 32, 16, big, None) == -2 and b"shorter than heads" in lib.ldt_last_error()
    # the entry points that were there keep their contracts
    assert lib.ldt_attention_bwd_cross(*args, 1, 2, 520, 8, 32, None) == -2 and b"Nq 520" in lib.ldt_last_error()


# ------------------------------------------------------------------------------------------------ the step and the trainer, on the CPU
def _compressor(tiny_cfg, **kw):
    import copy
    import ldt_amd
    c = copy.deepcopy(tiny_cfg.compressor)
    for k, v in kw.items():
        setattr(c, k, v)
    return ldt_amd.Compressor(c)


def test_refuse_undecodable_names_each_reason(tiny_cfg):
    from ldt_amd.compressor_train import DecoderTrainStep, refuse_undecodable
    refuse_undecodable(_compressor(tiny_cfg))                            # the tiny config itself is covered; parameters on the CPU
    for kw, msg in ((dict(class_condition=True, num_categorys=3), "class_condition"),
                    (dict(decoder_act="relu"), "decoder_act='relu'"),
                    (dict(norm="group_norm"), "norm='group_norm'.*layer_norm"),
                    (dict(max_outputs=None), "max_outputs: None.*mixture"),
                    (dict(decoder_dropout_p=0.1), "decoder_dropout_p=0.1"),
                    (dict(num_heads=4), "32-wide attention heads.*hidden 64 / 4 heads"),
                    (dict(z_scales=520), "64 set points on 520 latent tokens.*1 <= Nk <= 512")):
        with pytest.raises(NotImplementedError, match=msg):
            DecoderTrainStep(_compressor(tiny_cfg, **kw))
    m = _compressor(tiny_cfg)
    with pytest.raises(NotImplementedError, match="8200 set points on 8 latent tokens.*1 <= Nq <= 8192"):
        refuse_undecodable(m, num_points=8200)
    with pytest.raises(ValueError, match="100 set points from 64 prior rows"):
        refuse_undecodable(m, num_points=100)
    assert (DecoderTrainStep.MAX_QUERIES, DecoderTrainStep.MAX_KEYS) == (8192, 512)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DecoderTrainStep(m).forward(torch.zeros(2, 8, 120))
    with pytest.raises(RuntimeError, match="before forward"):
        DecoderTrainStep(m).backward(torch.zeros(2, 64, 3))


def test_decoder_parameters_are_the_decoder_side(tiny_cfg):
    from ldt_amd.compressor_train import decoder_parameters
    m = _compressor(tiny_cfg)
    names = [n for n, _ in decoder_parameters(m)]
    every = [n for n, _ in m.named_parameters()]
    assert names == [n for n in every if n in set(names)]                # module order
    assert "init_set.prior" in names and "output.weight" in names and "output.bias" in names
    for l in range(3):
        for leaf in ("ln.weight", "ln.bias", "att1.fc_q.weight", "att1.fc_kv.bias", "att1.fc_o.weight", "att1.norm1.norm.weight",
                     "att1.norm2.norm.bias", "att1.mlp.fc.0.0.weight", "att1.mlp.out.bias"):
            assert "decoder.%d.%s" % (l, leaf) in names
    rest = [n for n in every if n not in names]
    assert rest and all(n.startswith(("input.", "conv_in.", "encoder.", "group.", "pos_embedding.")) or ".att." in n or ".prior." in n for n in rest), rest
    assert len(names) == 3 + 3 * 16


def test_update_decoder_on_the_cpu_has_no_fallback_and_allocates_nothing(tiny_cfg):
    import ldt_amd
    tr = ldt_amd.CompressorTrainer(tiny_cfg, ldt_amd.Compressor(tiny_cfg.compressor), "cpu")
    assert tr.optimizer is None and tr.last_eps_grad is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.update_decoder({"tr_points": torch.zeros(2, 64, 3)})
    ct = ldt_amd.CompletionCompressorTrainer(tiny_cfg, ldt_amd.Compressor(tiny_cfg.compressor), "cpu")   # the completion trainer stays untouched
    with pytest.raises(NotImplementedError, match="CompletionCompressorTrainer.update_decoder.*CompressorTrainer alone"):
        ct.update_decoder({"tr_points": torch.zeros(2, 64, 3)})
    assert ct.optimizer is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.update_decoder({"tr_points": torch.zeros(2, 64, 3)}, eps=torch.zeros(2, 8, 120))
    assert tr.optimizer is None and tr.itr == 0 and all(p.grad is None for p in tr.model.parameters())
    with pytest.raises(NotImplementedError, match="not on this path"):   # update keeps refusing
        tr.update({})
    kw = [p.name for p in inspect.signature(ldt_amd.CompressorTrainer.update_decoder).parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert kw == ["eps", "post_noise"]
    bad = ldt_amd.CompressorTrainer(tiny_cfg, _compressor(tiny_cfg, decoder_act="relu"), "cpu")
    with pytest.raises(NotImplementedError, match="decoder_act"):
        bad.update_decoder({"tr_points": torch.zeros(2, 64, 3)})
    m = ldt_amd.Compressor(tiny_cfg.compressor)
    m._pack, m._pack_key = {"stale": 1}, ("k",)
    m.invalidate_packed()
    assert m._pack is None and m._pack_key is None
