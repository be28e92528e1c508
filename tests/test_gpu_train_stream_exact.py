"""GPU (-m gpu): the stream kernels of a Score training step (csrc/score_bwd.hip, csrc/optim.hip) at width and past their grid caps.

test_gpu_train_kernels.py holds each of them per element at one geometry: C = 128, contiguous operands, sizes a capped grid covers in one
sweep, row counts that are multiples of 4, beta1 = 0.9 from zero state.  Here every kernel runs at the smallest shapes that reach what
training reaches: hidden 1024 (16 lane passes, 16 column chunks) and MLP width 4096, a second sweep of every grid-stride loop with a tail
of 259, M % 4 = 1, 1 / 7 / 17 rows per sample, widths below 64, every row operand a column block of a wider buffer with its own row
stride, every destination inside sentinel, at::lerp's second form, no EMA, a late optimizer state with |g| over sixteen decades.

The cases, the references' bounds (kernel_checks.py, unchanged but for adam_ema_ref's stated moment_rounding term at the late state) and
the check functions are train_stream_checks'; test_train_stream_host.py shows on the CPU that a faithful fp32 emulation passes each check
and every planted index, stride, tail and branch fault fails it.  Every test prints its worst err / tol (-s); test_zz_margins prints the
worst per kernel, which DESIGN.md section 4.11 records."""
import collections

import pytest
import torch

import train_stream_checks as ts
from train_stream_checks import blk

pytestmark = pytest.mark.gpu

ops = None
RATIOS = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _mods():
    global ops
    assert torch.cuda.is_available()
    from ldt_amd import ops as ops_
    ops = ops_
    yield
    torch.cuda.empty_cache()


def report(kernel, name, ratio):
    RATIOS[kernel] = max(RATIOS[kernel], ratio)
    print("train-stream %-52s max err/tol %.3f" % (name, ratio))
    return ratio


def dev(c, *names):
    return [c[n].cuda() for n in names]


# ------------------------------------------------------------------------------------------------ LayerNorm + modulate backward
def ln_gpu(c, use_scale=True, want_mod=True):
    at = c["at"]
    x, dy, dxb, mod, dmod = dev(c, "x", "dy", "dx", "mod", "dmod")
    res = ops.layernorm_modulate_bwd(blk(x, at["x"]), blk(dy, at["dy"]), blk(dxb, at["dx"]), scale=blk(mod, at["scale"]) if use_scale else None,
                                     mod_sample_stride=6 * c["C"], rows_per_sample=c["rps"], want_mod=want_mod,
                                     dshift=blk(dmod, at["dshift"]) if want_mod else None, dscale=blk(dmod, at["dscale"]) if want_mod else None)
    assert want_mod or res == (None, None)
    return {"dx": dxb.cpu(), "dmod": dmod.cpu()}


@pytest.mark.parametrize("M,rps,C,offset", [s + (0.0,) for s in ts.LN_GATE_SHAPES] + [ts.LN_OFFSET_CASE])
def test_layernorm_modulate_bwd_at_width_strided_guarded(M, rps, C, offset):
    """(21, 7, 1024): M % 4 = 1, slices 7-15 idle, 16 lane passes and column chunks (also at mean^2 / variance ~ 100); (34, 17, 120): slice 0
    carries two rows, a 56-column tail chunk; (5, 1, 40): one row per sample, lanes 40-63 never load.  Then without scale and modulation
    outputs (the row kernel alone), and a second run of each: the same bits."""
    c = ts.ln_gate_case(M, rps, C, offset)
    out = ln_gpu(c)
    r = ts.ln_check(c, out)
    out0 = ln_gpu(c, use_scale=False, want_mod=False)
    r0 = ts.ln_check(c, out0, use_scale=False, want_mod=False)
    report("layernorm_modulate_bwd", "layernorm_modulate_bwd M%d rps%d C%d off%g" % (M, rps, C, offset), r)
    report("layernorm_modulate_bwd", "layernorm_modulate_bwd M%d rps%d C%d off%g, no scale" % (M, rps, C, offset), r0)
    again, again0 = ln_gpu(c), ln_gpu(c, use_scale=False, want_mod=False)
    assert all(torch.equal(again[k], out[k]) and torch.equal(again0[k], out0[k]) for k in out)


# ------------------------------------------------------------------------------------------------ gated residual backward
def gate_gpu(c, a_bf16, broadcast=False, want_dgate=True):
    at = c["at"]
    dy, a, dab, mod, dmod = dev(c, "dy", "a16" if a_bf16 else "a", "da", "mod", "dmod")
    gate = blk(mod, at["gate"])
    da, dg = ops.gate_residual_bwd(blk(dy, at["dy"]), gate[:1] if broadcast else gate, blk(a, at["a"]) if want_dgate else None,
                                   rows_per_sample=c["rps"], out=blk(dab, at["da"]), dgate=blk(dmod, at["dgate"]) if want_dgate else None)
    assert want_dgate or dg is None
    return {"da": dab.cpu(), "dmod": dmod.cpu()}


@pytest.mark.parametrize("M,rps,C", ts.LN_GATE_SHAPES)
@pytest.mark.parametrize("a_bf16", [False, True])
def test_gate_residual_bwd_at_width_strided_guarded(M, rps, C, a_bf16):
    """The shapes of the LayerNorm test; dy, a and da with three row strides; one gate row per sample, then one broadcast row
    (gate_sample_stride 0), then da alone."""
    c = ts.ln_gate_case(M, rps, C)
    out = gate_gpu(c, a_bf16)
    name = "gate_residual_bwd M%d rps%d C%d %s" % (M, rps, C, "bf16" if a_bf16 else "fp32")
    report("gate_residual_bwd", name, ts.gate_check(c, out, a_bf16))
    report("gate_residual_bwd", name + ", broadcast gate", ts.gate_check(c, gate_gpu(c, a_bf16, broadcast=True), a_bf16, broadcast=True))
    alone = gate_gpu(c, a_bf16, want_dgate=False)
    report("gate_residual_bwd", name + ", da alone", ts.gate_check(c, alone, a_bf16, want_dgate=False))
    assert torch.equal(alone["da"], out["da"])
    again = gate_gpu(c, a_bf16)
    assert torch.equal(again["da"], out["da"]) and torch.equal(again["dmod"], out["dmod"])


# ------------------------------------------------------------------------------------------------ GELU, SiLU, loss
@pytest.mark.parametrize("M,C,strided", ts.GELU_SHAPES)
@pytest.mark.parametrize("dh_bf16", [False, True])
def test_gelu_bwd_past_the_cap(M, C, strided, dh_bf16):
    """1,052,672 and 1,059,310 elements: a second sweep of the 4096 x 256 grid, which holds the edge values (+-12, +-6, +-3, +-0) of the last row."""
    c = ts.gelu_case(M, C, strided, dh_bf16)
    at = c["at"]
    u, dh, outb = dev(c, "u", "dh", "out")
    ops.gelu_bwd(blk(u, at["u"]), blk(dh, at["dh"]), out=blk(outb, at["out"]))
    report("gelu_bwd", "gelu_bwd %dx%d %s%s" % (M, C, "bf16" if dh_bf16 else "fp32", ", strided" if strided else ""), ts.gelu_check(c, {"out": outb.cpu()}))


@pytest.mark.parametrize("want_act", [False, True])
def test_silu_bwd_past_the_cap(want_act):
    """n = 524,288 + 259: one full sweep of the 2048 x 256 grid and a tail, the +-30 / +-0 values in the tail."""
    c = ts.silu_case()
    cd, dy = dev(c, "c", "dy")
    res = ops.silu_bwd(cd, dy, want_act=want_act)
    out = {"dc": res[0].cpu(), "act": res[1].cpu()} if want_act else {"dc": res.cpu()}
    report("silu_bwd", "silu_bwd n%d act=%d" % (c["n"], want_act), ts.silu_check(c, out, want_act))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("l1", [False, True])
def test_dsm_loss_bwd_past_the_cap(weighted, l1):
    """B = 3 samples of 174,849: the third sample's elements run across the end of the first sweep, where d = 0 elements are planted."""
    c = ts.dsm_case()
    eta, params, w = dev(c, "eta", "params", "w")
    out = ops.dsm_loss_bwd(eta, params, w if weighted else None, l1=l1)
    report("dsm_loss_bwd", "dsm_loss_bwd n%d w=%d l1=%d" % (c["n"], weighted, l1), ts.dsm_check(c, {"dparams": out.cpu()}, weighted, l1))


# ------------------------------------------------------------------------------------------------ column sum, embedding, cast
@pytest.mark.parametrize("M,C,wide", ts.COLSUM_CASES)
def test_colsum_at_width_guarded(M, C, wide):
    c = ts.colsum_case(M, C, wide)
    dy, outb = dev(c, "dy", "out")
    run = lambda buf: ops.colsum(blk(dy, c["at"]), out=buf[ts.GUARD:ts.GUARD + C])
    run(outb)
    report("colsum", "colsum %dx%d %s" % (M, C, "bf16 column block" if wide else "fp32"), ts.colsum_check(c, {"out": outb.cpu()}))
    again = c["out"].cuda()
    run(again)
    assert torch.equal(again, outb)


@pytest.mark.parametrize("B,D,K,ld,labels", ts.EMB_CASES)
def test_embedding_grad_blocks_and_stride(B, D, K, ld, labels):
    """D = 1024: four 256-column blocks from rows of stride 1032; D = 300: a partial second block.  One class without a sample in each."""
    c = ts.emb_case(B, D, K, ld, labels)
    dc, label = dev(c, "dc", "label")
    out = ops.embedding_grad(blk(dc, c["at"]), label, K)
    report("embedding_grad", "embedding_grad B%d D%d K%d ld%d" % (B, D, K, ld), ts.emb_check(c, {"dE": out.cpu()}))
    assert torch.equal(ops.embedding_grad(blk(dc, c["at"]), label, K), out)


@pytest.mark.parametrize("R,C", ts.TRANSPOSE_SHAPES)
@pytest.mark.parametrize("src_bf16", [False, True])
def test_transpose_cast_small_tiles(R, C, src_bf16):
    """(1, 40): one source row, two column tiles; (33, 33): 2 x 2 tiles, three of them one element wide or high."""
    c = ts.transpose_case(R, C, src_bf16)
    src, dstb = dev(c, "src", "dst")
    ops.transpose_cast_bf16(blk(src, c["at_src"]), rows_pad=c["Rp"], out=blk(dstb, c["at_dst"]))
    ts.transpose_check(c, {"dst": dstb.cpu()})
    assert torch.equal(ops.transpose_cast_bf16(blk(src, c["at_src"])).cpu(), c["want"])


# ------------------------------------------------------------------------------------------------ Adam + EMA
def adam_gpu_stepper(c):
    def step_(bufs, grad, step, ema_init):
        n, h = c["n"], ts.ADAM_HYPER
        d = {k: v.cuda() for k, v in bufs.items() if k != "guard"}
        g = grad.cuda()
        ops.adam_ema_step_(d["p"][:n], g, d["m"][:n], d["v"][:n], d["ema"][:n] if c["ema"] else None, step, h["lr"], c["b1"], h["b2"], h["eps"],
                           c["wd"], h["decay"], ema_init=ema_init)
        assert torch.equal(g.cpu(), grad)                                              # no clip factor: the gradient is left alone
        out = {k: v.cpu() for k, v in d.items()}
        if "guard" in bufs:
            out["guard"] = bufs["guard"]
        return out
    return step_


def test_adam_ema_step_past_the_cap_late_state():
    """n = 2 x 1,048,576 + 259, one step at step 100000 (bias corrections ~ 1, m and v far from zero, |g| from 1e-12 to 1e4): the second and
    third sweeps, 64 elements with g = m = v = 0 whose p must come back bit-identical, the buffers' tails intact, exp_avg and exp_avg_sq bit
    for bit the spelled-out fp32 chain."""
    c = ts.adam_main_case()
    report("adam_ema_step", "adam_ema_step n%d step 100000" % c["n"], ts.adam_run(c, adam_gpu_stepper(c)))


@pytest.mark.parametrize("variant", ts.ADAM_VARIANTS)
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_ema_step_lerp_form_2_and_no_ema(variant, wd):
    """lerp2: beta1 = 0.4, w1 = 0.6 >= 0.5 — at::lerp's second form; no_ema: ema = None, as AdamEMA.step without apply_ema.  Three steps from
    zero state each, every step from the device's own previous state."""
    c = ts.adam_variant_case(variant, wd)
    report("adam_ema_step", "adam_ema_step n%d %s wd%g" % (c["n"], variant, wd), ts.adam_run(c, adam_gpu_stepper(c)))


def test_zz_margins():
    """Printed last (DESIGN.md section 4.11 quotes them): the worst err / tol per kernel over this file's cases."""
    for k in sorted(RATIOS):
        print("worst err / tol, %-28s %.3f" % (k + ":", RATIOS[k]))
        assert RATIOS[k] <= 1.0
