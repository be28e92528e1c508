"""CPU: the checks of test_gpu_train_stream_exact.py have teeth, and their bounds are not too tight at width.

For every case of the GPU file, (a) the faithful fp32 emulation of the kernel (train_stream_checks.*_emu: the kernel's own order of
operations, strides, sweeps, slices and row groups) passes the very check function the GPU test applies to the device's output, and (b) every
planted fault that can show at that case fails it: an element outside the reference's bound, a changed sentinel, or — for Adam's moments,
which the kernel spells out operation by operation — a changed bit."""
import pytest
import torch

import train_stream_checks as ts


def caught(check, what):
    with pytest.raises(AssertionError):
        check()
        print("NOT CAUGHT: " + what)


# ------------------------------------------------------------------------------------------------------------- the helpers themselves
def test_fma32x_is_the_single_rounding():
    """Where float64's own rounding of a b + c lands on an fp32 rounding boundary, (a b + c).float() rounds twice; fma32x must not."""
    a = torch.tensor([1.0 + 2.0 ** -23, 3.0, 1.0, 1.0])
    b = torch.tensor([1.0 + 2.0 ** -23, 0.5, 2.0 ** -24, 2.0 ** -24])
    c = torch.tensor([2.0 ** -60, 0.25, 1.0, 1.0 + 2.0 ** -23])
    # exact: 1 + 2^-22 + 2^-46 + 2^-60 -> 1 + 2^-22;  1.75;  1 + 2^-24 (tie -> even, 1);  1 + 2^-23 + 2^-24 (tie -> even, 1 + 2^-22)
    want = torch.tensor([1.0 + 2.0 ** -22, 1.75, 1.0, 1.0 + 2.0 ** -22])
    assert torch.equal(ts.fma32x(a, b, c), want)
    # a b = 2^-24 - 2^-70, c = 1 + 2^-23: the exact sum lies 2^-70 BELOW the fp32 tie and rounds down to c; float64 rounds it onto the tie,
    # and the tie then goes to even, one ulp up
    a2, b2, c2 = torch.tensor([2.0 ** -12 * (1 + 2.0 ** -23)]), torch.tensor([2.0 ** -12 * (1 - 2.0 ** -23)]), torch.tensor([1.0 + 2.0 ** -23])
    assert torch.equal(ts.fma32x(a2, b2, c2), c2)
    assert torch.equal((a2.double() * b2.double() + c2.double()).float(), torch.tensor([1.0 + 2.0 ** -22]))


def test_lane_sum_and_slice_sum_orders():
    g = ts.gen(1)
    v = torch.randn(3, 200, generator=g)
    s = ts.lane_sum(v)
    assert s.shape == (3, 1) and float((s[:, 0].double() - v.double().sum(1)).abs().max()) < 200 * 2.0 ** -24 * float(v.abs().sum(1).max())
    ones = torch.ones(2, 40)
    assert torch.equal(ts.lane_sum(ones), torch.full((2, 1), 40.0))
    t = torch.arange(2 * 17 * 3, dtype=torch.float32).reshape(2, 17, 3)
    assert torch.equal(ts.slice_sum(t), t.double().sum(1))
    assert torch.equal(ts.slice_sum(t, fault="drop_slices"), t.double()[:, [0, 1, 2, 3, 4, 5, 6, 7, 16]].sum(1))


# ------------------------------------------------------------------------------------------------------------- LayerNorm + modulate, gate
LN_RUNS = [s + (0.0,) for s in ts.LN_GATE_SHAPES] + [ts.LN_OFFSET_CASE]


@pytest.mark.parametrize("M,rps,C,offset", LN_RUNS)
def test_layernorm_modulate_bwd_emulation_and_faults(M, rps, C, offset):
    c = ts.ln_gate_case(M, rps, C, offset)
    r = ts.ln_check(c, ts.ln_emu(c))
    r0 = ts.ln_check(c, ts.ln_emu(c, use_scale=False, want_mod=False), use_scale=False, want_mod=False)
    print("host layernorm_modulate_bwd M%d rps%d C%d off%g: emulation err/tol %.3f (no scale %.3f)" % (M, rps, C, offset, r, r0))
    faults = ts.ln_faults_of(c)
    assert ("skip_row_tail" in faults) == (M % 4 != 0) and ("drop_slices" in faults) == (rps > 8) and ("tail_lane" in faults) == (C % 64 != 0)
    for f in faults:
        caught(lambda: ts.ln_check(c, ts.ln_emu(c, fault=f)), "layernorm_modulate_bwd " + f)
    for f in [f for f in faults if f != "drop_slices"]:                                 # the row kernel alone
        caught(lambda: ts.ln_check(c, ts.ln_emu(c, use_scale=False, want_mod=False, fault=f), use_scale=False, want_mod=False), "no scale " + f)


@pytest.mark.parametrize("M,rps,C", ts.LN_GATE_SHAPES)
@pytest.mark.parametrize("a_bf16", [False, True])
def test_gate_residual_bwd_emulation_and_faults(M, rps, C, a_bf16):
    c = ts.ln_gate_case(M, rps, C)
    r = ts.gate_check(c, ts.gate_emu(c, a_bf16), a_bf16)
    rb = ts.gate_check(c, ts.gate_emu(c, a_bf16, broadcast=True), a_bf16, broadcast=True)
    rn = ts.gate_check(c, ts.gate_emu(c, a_bf16, want_dgate=False), a_bf16, want_dgate=False)
    print("host gate_residual_bwd M%d rps%d C%d bf16=%d: emulation err/tol %.3f (broadcast %.3f, da alone %.3f)" % (M, rps, C, a_bf16, r, rb, rn))
    for f in ts.gate_faults_of(c):
        caught(lambda: ts.gate_check(c, ts.gate_emu(c, a_bf16, fault=f), a_bf16), "gate_residual_bwd " + f)
    # a kernel that took the sample's own row where one broadcast row is passed, and the reverse
    caught(lambda: ts.gate_check(c, ts.gate_emu(c, a_bf16), a_bf16, broadcast=True), "gate_residual_bwd broadcast ignored")
    caught(lambda: ts.gate_check(c, ts.gate_emu(c, a_bf16, broadcast=True), a_bf16), "gate_residual_bwd always broadcast")


# ------------------------------------------------------------------------------------------------------------- the grid-stride kernels
@pytest.mark.parametrize("M,C,strided", ts.GELU_SHAPES)
@pytest.mark.parametrize("dh_bf16", [False, True])
def test_gelu_bwd_emulation_and_faults(M, C, strided, dh_bf16):
    c = ts.gelu_case(M, C, strided, dh_bf16)
    print("host gelu_bwd %dx%d bf16=%d: emulation err/tol %.3f" % (M, C, dh_bf16, ts.gelu_check(c, ts.gelu_emu(c))))
    for f in ts.gelu_faults_of(c):
        caught(lambda: ts.gelu_check(c, ts.gelu_emu(c, fault=f)), "gelu_bwd " + f)
    # the planted edge values are out of the first sweep's reach: a loop one thread short of the whole still misses one of them
    caught(lambda: ts.gelu_check(c, ts.gelu_emu(c, fault="first_sweep", sweep=(M - 1) * C + 7)), "gelu_bwd last edge value")


@pytest.mark.parametrize("want_act", [False, True])
def test_silu_bwd_emulation_and_faults(want_act):
    c = ts.silu_case()
    print("host silu_bwd act=%d: emulation err/tol %.3f" % (want_act, ts.silu_check(c, ts.silu_emu(c, want_act), want_act)))
    caught(lambda: ts.silu_check(c, ts.silu_emu(c, want_act, fault="first_sweep"), want_act), "silu_bwd first_sweep")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("l1", [False, True])
def test_dsm_loss_bwd_emulation_and_faults(weighted, l1):
    c = ts.dsm_case()
    print("host dsm_loss_bwd w=%d l1=%d: emulation err/tol %.3f" % (weighted, l1, ts.dsm_check(c, ts.dsm_emu(c, weighted, l1), weighted, l1)))
    for f in ts.dsm_faults_of(weighted):
        caught(lambda: ts.dsm_check(c, ts.dsm_emu(c, weighted, l1, fault=f), weighted, l1), "dsm_loss_bwd " + f)


# ------------------------------------------------------------------------------------------------------------- column sum, embedding, cast
@pytest.mark.parametrize("M,C,wide", ts.COLSUM_CASES)
def test_colsum_emulation_and_faults(M, C, wide):
    c = ts.colsum_case(M, C, wide)
    print("host colsum %dx%d: emulation err/tol %.3f" % (M, C, ts.colsum_check(c, ts.colsum_emu(c))))
    for f in ts.colsum_faults_of(c):
        caught(lambda: ts.colsum_check(c, ts.colsum_emu(c, fault=f)), "colsum " + f)


@pytest.mark.parametrize("B,D,K,ld,labels", ts.EMB_CASES)
def test_embedding_grad_emulation_and_faults(B, D, K, ld, labels):
    c = ts.emb_case(B, D, K, ld, labels)
    assert len(c["absent"]) == 1
    print("host embedding_grad B%d D%d: emulation err/tol %.3f" % (B, D, ts.emb_check(c, ts.emb_emu(c))))
    for f in ts.emb_faults_of(c):
        caught(lambda: ts.emb_check(c, ts.emb_emu(c, fault=f)), "embedding_grad " + f)


@pytest.mark.parametrize("R,C", ts.TRANSPOSE_SHAPES)
@pytest.mark.parametrize("src_bf16", [False, True])
def test_transpose_cast_emulation_and_faults(R, C, src_bf16):
    c = ts.transpose_case(R, C, src_bf16)
    ts.transpose_check(c, ts.transpose_emu(c))
    if R > 1:                                                                           # (one row has no row stride to get wrong)
        caught(lambda: ts.transpose_check(c, ts.transpose_emu(c, fault="ld_is_C")), "transpose_cast ld_is_C")
    caught(lambda: ts.transpose_check(c, {"dst": c["dst"]}), "transpose_cast nothing written")
    spill = ts.transpose_emu(c)
    spill["dst"][1, c["Rp"]] = 0                                                        # one zero too many to the right of the padding
    caught(lambda: ts.transpose_check(c, spill), "transpose_cast writes past R_pad")


# ------------------------------------------------------------------------------------------------------------- Adam + EMA
def _emu_stepper(c, fault=None):
    return lambda bufs, grad, step, ema_init: ts.adam_emu(c, bufs, grad, step, ema_init, fault=fault)


def test_adam_main_case_emulation_and_faults():
    c = ts.adam_main_case()
    assert ts.adam_faults_of(c) == ["first_sweep"]
    print("host adam_ema_step main: emulation err/tol %.3f" % ts.adam_run(c, _emu_stepper(c)))
    caught(lambda: ts.adam_run(c, _emu_stepper(c, "first_sweep")), "adam_ema_step first_sweep")

    def moved(bufs, grad, step, ema_init):                                              # p of the all-zero block off by one ulp: inside any bound
        out = ts.adam_emu(c, bufs, grad, step, ema_init)
        z0 = c["zero"][0]
        out["p"][z0] = torch.nextafter(out["p"][z0], torch.tensor(float("inf")))
        return out
    caught(lambda: ts.adam_run(c, moved), "adam_ema_step zero block")


@pytest.mark.parametrize("variant", ts.ADAM_VARIANTS)
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_variants_emulation_and_faults(variant, wd):
    c = ts.adam_variant_case(variant, wd)
    faults = ts.adam_faults_of(c)
    assert faults == (["lerp_form"] if variant == "lerp2" else ["ema_absent"])
    print("host adam_ema_step %s wd%g: emulation err/tol %.3f" % (variant, wd, ts.adam_run(c, _emu_stepper(c))))
    for f in faults:
        caught(lambda: ts.adam_run(c, _emu_stepper(c, f)), "adam_ema_step " + f)
