"""CPU: the references and bounds of the fp32 linear's tests (sgemm_checks.py) judged without a GPU.

fp32 emulations of the seven kernel forms in each kernel's own order (sgemm_checks.emulate: FMA chains for the scalar and streaming forms,
k / k + 4 pairs per 8-k group for the MFMA forms, per-lane partial sums and five xor-shuffle additions for the small-N form) must pass every
check that test_gpu_sgemm_exact.py applies to the HIP kernels, on every case of the table (rows reduced where speed needs it, the grid cap
lowered with them so that the later trips of the streaming forms are still taken).  The same emulation with one planted fault must FAIL: the
proof that the derived bounds tell a right kernel from a nearly right one.  The conditions on the inputs of the bf16 cases (ambiguous and
unresolved shares) are asserted here from the reference alone."""
import pytest
import torch

import kernel_checks as kc
import sgemm_checks as sc

CASE_IDS = [c.name for c in sc.SGEMM_CASES]
EMU_CUS = 1                                       # the emulated device: one CU, so a few thousand rows already take a second trip


def reduced(case, budget=40000):
    """-> M' <= M: enough rows for two passes of the emulated grid and a ragged tail where the form strides over the rows, else about
    `budget` outputs"""
    per_pass = sc.rows_per_pass(case.route, case.N, EMU_CUS)
    if per_pass is not None:
        return min(case.M, per_pass + 5 if per_pass * case.N <= 4 * budget else max(40, budget // case.N))
    return min(case.M, max(8, budget // case.N))


def inputs(case, rows=None, coherent=False):
    a, w, bias = sc.case_inputs(case, coherent)
    return a[:rows or reduced(case)].clone(), w, bias


@pytest.mark.parametrize("case", sc.SGEMM_CASES, ids=CASE_IDS)
def test_emulation_of_every_form_passes_the_bounds(case):
    pre = {}
    worst = 0.0
    for with_bias, act_in, act_out, bf16 in sc.operand_sets(case):
        a, w, bias = inputs(case, coherent=sc.coherent(case, bf16))
        b = bias if with_bias else None
        if (with_bias, act_in, sc.coherent(case, bf16)) not in pre:
            pre[(with_bias, act_in, sc.coherent(case, bf16))] = sc.pre_activation(a, w, b, act_in)
        ref, tol = sc.activated(*pre[(with_bias, act_in, sc.coherent(case, bf16))], act_out)
        out = sc.emulate(case.route, a, w, b, act_in, act_out, bf16, cus=EMU_CUS)
        worst = max(worst, sc.check(out, ref, tol, "emulated %s: bias %s in %d out %d bf16 %s" % (case.name, with_bias, act_in, act_out, bf16)))
    print("worst err / tol %.3f (emulated %s)" % (worst, case.name))


@pytest.mark.parametrize("case", sc.SGEMM_CASES, ids=CASE_IDS)
def test_emulation_is_exact_on_the_probes(case):
    M, N, K = reduced(case), case.N, case.K
    x, w, ref = kc.selection_probe(M, N, K)
    b = (torch.arange(N) % 7 - 3).float()
    kc.assert_elementwise(sc.emulate(case.route, x, w, b), ref.double() + b.double(), 0.0, "selection probe, emulated %s" % case.name)
    x, wi, bi, iref = kc.integer_probe(M, N, K, seed=M + N + K)
    kc.assert_elementwise(sc.emulate(case.route, x, wi, bi), iref, 0.0, "integer probe, emulated %s" % case.name)


@pytest.mark.parametrize("case", sc.SGEMM_CASES, ids=CASE_IDS)
def test_bf16_cases_meet_their_conditions_from_the_reference_alone(case):
    """AMBIGUOUS_CAP (2 %) and UNRESOLVED_CAP (3 %) are conditions on the inputs: asserted here on the CPU for every bf16 operand set of every
    case, on the first rows (up to about a million outputs) of the very inputs the GPU test uses."""
    rows = min(case.M, max(64, 1000000 // case.N))
    a, w, bias = inputs(case, rows, coherent=sc.coherent(case, True))
    for with_bias, act_in, act_out, bf16 in sc.operand_sets(case):
        if not bf16:
            continue
        assert act_out != sc.ACT_GELU or case.K <= sc.GELU_BF16_MAX_K
        ref, tol = sc.reference(a, w, bias if with_bias else None, act_in, act_out)
        _, ambiguous, unresolved = sc.bf16_shares(ref, tol)
        print("%s bias %s in %s out %s: ambiguous %.4f unresolved %.4f" % (case.name, with_bias, sc.ACT_NAMES[act_in], sc.ACT_NAMES[act_out], ambiguous, unresolved))
        assert ambiguous <= kc.AMBIGUOUS_CAP and unresolved <= sc.UNRESOLVED_CAP, (case.name, with_bias, act_in, act_out, ambiguous, unresolved)


def test_relu_output_is_exactly_zero_where_the_sum_is_negative_for_certain():
    a, w, bias = inputs(sc.CASE["mfma128-129x129x20"])
    pre, tol_pre = sc.pre_activation(a, w, bias, sc.ACT_NONE)
    ref, tol = sc.activated(pre, tol_pre, sc.ACT_RELU)
    sure = pre < -tol_pre
    assert bool(sure.any()) and float(tol[sure].max()) == 0 and float(ref[sure].abs().max()) == 0 and bool((tol[~sure] > 0).all())
    out = sc.emulate(sc.ROUTE_MFMA_128, a, w, bias, act_out=sc.ACT_RELU)
    sc.check(out, ref, tol, "relu")
    out[torch.nonzero(sure)[0][0], torch.nonzero(sure)[0][1]] = 1e-30           # a denormal-sized leak through the select
    with pytest.raises(AssertionError):
        sc.check(out, ref, tol, "relu, leaked")


def test_the_activation_bounds_hold_on_a_dense_sweep():
    """silu_ref / gelu_ref's own-error terms against the fp32 evaluation (emulated), |x| up to 100: the counts are bounds, not fits"""
    x = torch.cat([torch.linspace(-100, 100, 400001), torch.tensor(sc.SPECIAL_ROW_VALUES)]).float()
    for act, f in ((sc.ACT_SILU, sc.silu_ref), (sc.ACT_GELU, sc.gelu_ref)):
        ref, err = f(x.double())
        got = sc._act32(x, act).double()
        assert bool(((got - ref).abs() <= err).all()), act


# ------------------------------------------------------------------------------------------------------------- planted faults
# (fault, case, rows, operand set (bias, act_in, act_out, bf16)): the check must pass without the fault and fail with it
FAULTS = [
    ("no_second_trip", "smalln4-262157x2x4", None, (True, 0, 0, False)),
    ("no_second_trip", "smalln8-131079x6x8", None, (True, 0, 0, False)),
    ("no_second_trip", "smallk4-20000x1024x3", None, (True, 0, 0, False)),
    ("no_second_trip", "smallk8-16389x512x6", None, (True, 0, sc.ACT_SILU, True)),
    ("tail_overwrites_last", "smallk4-20001x128x3", None, (True, 0, 0, False)),
    ("tail_overwrites_last", "smalln4-8195x3x132", None, (True, 0, 0, False)),
    ("tail_unwritten", "smallk8-8197x32x7", None, (True, 0, 0, False)),
    ("tail_unwritten", "smalln8-8194x7x136", None, (False, 0, 0, True)),
    ("drop_ragged_k", "mfma32-33x200x36", None, (True, 0, 0, False)),
    ("drop_ragged_k", "mfma128-129x129x20", None, (True, 0, 0, False)),
    ("drop_ragged_k", "nt-130x131x21", None, (True, 0, 0, False)),
    ("drop_ragged_k", "smalln4-8195x3x132", None, (True, 0, 0, False)),
    ("bias_next", "mfma128-49x84x8", None, (True, 0, 0, False)),
    ("bias_next", "smallk4-8201x64x4", None, (True, 0, sc.ACT_SILU, True)),
    ("silu_after", "mfma32-19x2085x512", None, (False, sc.ACT_SILU, 0, False)),
    ("silu_after", "smalln4-8200x4x128", None, (False, sc.ACT_SILU, 0, False)),
    ("act_before_bias", "nt-70x70x4", None, (True, 0, sc.ACT_SILU, True)),
    ("act_before_bias", "smallk8-8192x128x5", None, (True, 0, sc.ACT_GELU, True)),
    ("bf16_truncate", "mfma128-200x136x36", None, (True, 0, sc.ACT_GELU, True)),
    ("bf16_truncate", "smallk4-8192x32x1", None, (True, 0, sc.ACT_SILU, True)),
    ("perm_one_operand", "mfma128-130x300x256", None, (True, 0, 0, False)),
    ("perm_one_operand", "mfma32-48x86x8", None, (False, sc.ACT_SILU, 0, False)),
    ("store_shift4", "smallk4-8199x1024x2", None, (True, 0, 0, False)),
    ("store_shift4", "smallk8-8203x256x8", None, (True, 0, sc.ACT_SILU, True)),
]


@pytest.mark.parametrize("fault,name,rows,ops_set", FAULTS, ids=["%s-%s" % (f[0], f[1]) for f in FAULTS])
def test_planted_fault_is_caught_by_the_per_element_check(fault, name, rows, ops_set):
    case = sc.CASE[name]
    with_bias, act_in, act_out, bf16 = ops_set
    assert ops_set in sc.operand_sets(case), "the fault must be caught by an operand set the GPU test runs on this case"
    a, w, bias = inputs(case, rows, coherent=sc.coherent(case, bf16))
    b = bias if with_bias else None
    ref, tol = sc.reference(a, w, b, act_in, act_out)
    sc.check(sc.emulate(case.route, a, w, b, act_in, act_out, bf16, cus=EMU_CUS), ref, tol, "sound")
    with pytest.raises(AssertionError):
        sc.check(sc.emulate(case.route, a, w, b, act_in, act_out, bf16, fault=fault, cus=EMU_CUS), ref, tol, fault)


@pytest.mark.parametrize("fault,name", [("no_second_trip", "smallk4-8199x1024x2"), ("no_second_trip", "smalln8-131079x6x8"),
                                        ("tail_unwritten", "smalln4-262157x2x4"), ("bias_next", "nt-5x64x3"), ("drop_ragged_k", "mfma32-33x200x36"),
                                        ("perm_one_operand", "mfma128-129x129x20"), ("store_shift4", "smallk8-16389x512x6")])
def test_planted_fault_is_caught_by_an_exact_probe(fault, name):
    """the probes see what needs no bound: rows or columns in the wrong place, a bias of the wrong column, terms that are missing"""
    case = sc.CASE[name]
    M, N, K = reduced(case), case.N, case.K
    x, w, ref = kc.selection_probe(M, N, K)
    b = (torch.arange(N) % 7 - 3).float()
    x2, wi, bi, iref = kc.integer_probe(M, N, K, seed=M + N + K)
    caught = 0
    for xx, ww, bb, want in ((x, w, b, ref.double() + b.double()), (x2, wi, bi, iref)):
        kc.assert_elementwise(sc.emulate(case.route, xx, ww, bb, cus=EMU_CUS), want, 0.0, "sound")
        try:
            kc.assert_elementwise(sc.emulate(case.route, xx, ww, bb, fault=fault, cus=EMU_CUS, fill=float("nan")), want, 0.0, fault)
        except AssertionError:
            caught += 1
    assert caught >= 1
