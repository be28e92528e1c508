"""GPU (-m gpu): every kernel form of the fp32 linear (ops.sgemm) per element, by route (helpers: tests/sgemm_checks.py on kernel_checks.py).

ldt_sgemm is one entry point with seven kernel forms behind it.  Every case of sgemm_checks.SGEMM_CASES first asserts the form the launcher's
own query (ops.sgemm_route) names, then holds the result (a) to a componentwise bound against float64 of act_out(act_in(a) . w^T + b) — bf16
outputs bit for bit where fp32 resolves a bf16 ulp —, (b) to equality on operands whose result is exact in any summation order, (c) to
bit-equality with the dense call when operands and output are aligned interiors of wider guarded buffers, and (d) to the bound again when one
operand at a time sits 4 bytes off alignment and the route changes under it."""
import collections

import pytest
import torch

import kernel_checks as kc
import sgemm_checks as sc

pytestmark = pytest.mark.gpu

ops = None
LdtHipError = None
RATIOS = collections.defaultdict(float)          # worst err / tol per route and activation (printed by test_zz_margins)
CASE_IDS = [c.name for c in sc.SGEMM_CASES]
REPRESENTATIVES = [sc.CASE[n] for n in sc.REPRESENTATIVES]
GUARD = 4096


@pytest.fixture(scope="module", autouse=True)
def _mods():
    global ops, LdtHipError
    assert torch.cuda.is_available()
    from ldt_amd import _lib, ops as _ops
    ops, LdtHipError = _ops, _lib.LdtHipError
    assert (_lib.ACT_NONE, _lib.ACT_SILU, _lib.ACT_RELU, _lib.ACT_GELU) == (sc.ACT_NONE, sc.ACT_SILU, sc.ACT_RELU, sc.ACT_GELU)
    torch.backends.cuda.matmul.allow_tf32 = False
    yield


def dev(x):
    return None if x is None else x.to("cuda")


def note(kind, ratio):
    RATIOS[kind] = max(RATIOS[kind], ratio)
    return ratio


def off4(t):
    """t's values in a fresh device buffer that starts 4 bytes past a 16-byte boundary (dense rows)"""
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def placed(case, a):
    return off4(a) if case.view == "a+4" else dev(a)


def key(route, act_in, act_out, bf16):
    if bf16:
        return "sgemm %s, bf16 out" % sc.ROUTE_NAMES[route]
    return "sgemm %s, in %s out %s" % (sc.ROUTE_NAMES[route], "silu" if act_in == sc.ACT_SILU else "-", sc.ACT_NAMES[act_out])


# ------------------------------------------------------------------------------------------------------------- per element
@pytest.mark.parametrize("case", sc.SGEMM_CASES, ids=CASE_IDS)
def test_sgemm_per_element(case):
    """One shape per route runs the full matrix (bias or none x act_in x act_out x fp32 / bf16); every other shape fp32 + bias, SiLU in without
    bias (the AdaLN form) and SiLU out -> bf16; bf16 + GELU wherever K <= 36.  randn inputs, weights / sqrt(K), one row of `a` holding +-30, +-0
    and +-88 (sc.case_inputs; same-sign inputs for the bf16 sets above K = 136, see sc.COHERENT_ABOVE_K).  The float64 pre-activation and its
    bound are computed once per (bias, act_in) and shared by the output activations."""
    data, pre = {}, {}
    for with_bias, act_in, act_out, bf16 in sc.operand_sets(case):
        co = sc.coherent(case, bf16)
        if co not in data:
            a, w, bias = sc.case_inputs(case, co)
            data[co] = placed(case, a), dev(w), dev(bias)
            assert ops.sgemm_route(*data[co]) == case.route
        a, w, bias = data[co]
        b = bias if with_bias else None
        if (with_bias, act_in, co) not in pre:
            pre[(with_bias, act_in, co)] = sc.pre_activation(a, w, b, act_in)
        ref, tol = sc.activated(*pre[(with_bias, act_in, co)], act_out)
        what = "sgemm %s (%s): bias %s, in %s, out %s, %s" % (case.name, sc.ROUTE_NAMES[case.route], with_bias, sc.ACT_NAMES[act_in],
                                                               sc.ACT_NAMES[act_out], "bf16" if bf16 else "fp32")
        out = ops.sgemm(a, w, b, act_in=act_in, act_out=act_out, out_bf16=bf16)
        r = note(key(case.route, act_in, act_out, bf16), sc.check(out, ref, tol, what))
        print("worst err / tol %.3f  %s" % (r, what))


# ------------------------------------------------------------------------------------------------------------- exact probes
@pytest.mark.parametrize("case", sc.SGEMM_CASES, ids=CASE_IDS)
def test_sgemm_exact_probes(case):
    """One-hot rows (a signed gather of w) and small integers (exact in any summation order), tolerance 0; past the grid cap of a streaming
    form once more with every nonzero row in the LAST trip of the grid-stride loop."""
    M, N, K = case.M, case.N, case.K
    x, w, ref = kc.selection_probe(M, N, K)
    b = (torch.arange(N) % 7 - 3).float()
    x = placed(case, x)
    assert ops.sgemm_route(x, dev(w), dev(b)) == case.route
    kc.assert_elementwise(ops.sgemm(x, dev(w), dev(b)), dev(ref).double() + dev(b).double(), 0.0, "selection probe, sgemm %s" % case.name)
    x, wi, bi, iref = kc.integer_probe(M, N, K, seed=M + N + K, device="cuda")
    kc.assert_elementwise(ops.sgemm(placed(case, x), dev(wi), dev(bi)), iref, 0.0, "integer probe, sgemm %s" % case.name)
    if case.name in sc.PAST_THE_CAP:
        per_pass = sc.rows_per_pass(case.route, N, cus=torch.cuda.get_device_properties(0).multi_processor_count)
        first = (M - 1) // per_pass * per_pass
        assert 0 < first < M, "%s is not past the grid cap of this device (%d rows per pass)" % (case.name, per_pass)
        x2 = torch.zeros_like(x)
        x2[first:] = x[first:]
        x2[first:, 0] = torch.where(x2[first:, 0] == 0, torch.ones(M - first), x2[first:, 0])       # (no row of the last trip is all zero)
        want = dev(x2).double() @ dev(wi).double().T + dev(bi).double()                              # small integers: exact
        assert bool((want == want.round()).all()) and float(want.abs().max()) <= 256
        kc.assert_elementwise(ops.sgemm(dev(x2), dev(wi), dev(bi)), want, 0.0, "integer probe in the last trip (rows %d..), sgemm %s" % (first, case.name))


# ------------------------------------------------------------------------------------------------------------- views
SENT_BF16 = torch.tensor(kc.SENT_F32).bfloat16()
FILL = 7.0                                        # what the output view holds before the call: the columns around the slice must keep it


def guarded(rows, cols, dtype, fill, offset=0):
    """kc.guarded for either output type, the view optionally `offset` elements past its aligned place.  -> (big, view, check()): check
    asserts that nothing outside the view's rows x cols elements was written."""
    sent = SENT_BF16.to("cuda") if dtype == torch.bfloat16 else torch.tensor(kc.SENT_F32, device="cuda")
    big = torch.empty(rows * cols + 2 * GUARD, dtype=dtype, device="cuda")
    big.fill_(sent)
    view = big[GUARD + offset:GUARD + offset + rows * cols].view(rows, cols)
    view.fill_(fill)
    assert view.data_ptr() % 16 == (offset * big.element_size()) % 16

    def check(what):
        lo, hi = big[:GUARD + offset], big[GUARD + offset + rows * cols:]
        bad = int((lo != sent).sum()) + int((hi != sent).sum())
        assert bad == 0, "%s: %d element(s) written outside the output buffer" % (what, bad)
    return big, view, check


def wide(t, pad):
    """t as columns pad .. pad + cols of a guarded fp32 buffer `2 pad` wider, NaN in the other columns.  -> (slice, check)"""
    _, v, check = guarded(t.shape[0], t.shape[1] + 2 * pad, torch.float32, float("nan"))
    v[:, pad:pad + t.shape[1]] = t
    return v[:, pad:pad + t.shape[1]], check


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", REPRESENTATIVES, ids=sc.REPRESENTATIVES)
def test_sgemm_strided_views_keep_the_route(case, bf16):
    """A, W and the output as 16-byte aligned column slices of wider guarded buffers (16 bytes in: 4 fp32 / 8 bf16 columns), as the product's
    out=mod[:, l*6*D:(l+1)*6*D]: the same route, the same bits as the dense call, within the bound, nothing written around the slice.  The
    bf16 run is the 8-byte-store case of the small-K form."""
    a, w, bias = (dev(t) for t in sc.case_inputs(case))
    M, N, K = case.M, case.N, case.K
    dense = ops.sgemm(a, w, bias, out_bf16=bf16)
    av, check_a = wide(a, 4)
    wv, check_w = wide(w, 4)
    pad = 8 if bf16 else 4
    _, o, check_o = guarded(M, N + 2 * pad, torch.bfloat16 if bf16 else torch.float32, FILL)
    ov = o[:, pad:pad + N]
    assert ov.data_ptr() % 16 == 0 and av.data_ptr() % 16 == 0 and wv.data_ptr() % 16 == 0
    assert ops.sgemm_route(av, wv, bias, ov) == case.route == ops.sgemm_route(a, w, bias)
    ops.sgemm(av, wv, bias, out=ov)
    what = "sgemm %s, strided views, %s" % (case.name, "bf16" if bf16 else "fp32")
    ref, tol = sc.reference(a, w, bias)
    note(key(case.route, 0, 0, bf16), sc.check(ov, ref, tol, what))
    assert torch.equal(ov, dense), what + ": differs from the dense call"
    for c in (check_a, check_w, check_o):
        c(what)
    assert bool((o[:, :pad] == FILL).all()) and bool((o[:, pad + N:] == FILL).all()), what + ": a column beside the slice was written"
    assert torch.equal(av, a) and torch.equal(wv, w)


def route_when_misaligned(route, which):
    """the alignment rules: the small-N and MFMA forms load 16 bytes from A and W, the small-K forms from bias and store 16 / 8 to C; the
    representatives of the small-K forms have K < 8, which no MFMA form takes: the scalar kernel it is"""
    if which in ("a", "w"):
        return sc.ROUTE_NT if route in (sc.ROUTE_MFMA_128, sc.ROUTE_MFMA_32, sc.ROUTE_SMALLN_4, sc.ROUTE_SMALLN_8) else route
    return sc.ROUTE_NT if route in (sc.ROUTE_SMALLK_4, sc.ROUTE_SMALLK_8) else route


@pytest.mark.parametrize("which", ["a", "w", "out", "bias"])
@pytest.mark.parametrize("case", REPRESENTATIVES, ids=sc.REPRESENTATIVES)
def test_sgemm_misaligned_views_change_the_route_not_the_result(case, which):
    """A 4-byte offset on A, then W, then out, then bias, one at a time: the query names the route (the scalar kernel wherever no other form's
    alignment rule still holds), the result stays within the bound, nothing is written outside the output."""
    a, w, bias = (dev(t) for t in sc.case_inputs(case))
    ref, tol = sc.reference(a, w, bias)
    av, wv, bv = (off4(a) if which == "a" else a), (off4(w) if which == "w" else w), (off4(bias) if which == "bias" else bias)
    _, ov, check_o = guarded(case.M, case.N, torch.float32, FILL, offset=1 if which == "out" else 0)
    got = ops.sgemm_route(av, wv, bv, ov)
    assert got == route_when_misaligned(case.route, which), (case.name, which, got)
    ops.sgemm(av, wv, bv, out=ov)
    what = "sgemm %s, %s 4 bytes off: %s" % (case.name, which, sc.ROUTE_NAMES[got])
    note(key(got, 0, 0, False), sc.check(ov, ref, tol, what))
    check_o(what)


@pytest.mark.parametrize("case", REPRESENTATIVES, ids=sc.REPRESENTATIVES)
def test_sgemm_repeats_bit_for_bit(case):
    a, w, bias = (dev(t) for t in sc.case_inputs(case))
    first = ops.sgemm(a, w, bias, act_in=sc.ACT_SILU, act_out=sc.ACT_GELU)
    assert torch.equal(ops.sgemm(a, w, bias, act_in=sc.ACT_SILU, act_out=sc.ACT_GELU), first)


def test_sgemm_route_none_is_a_refusal():
    """route 0: the query says no kernel takes the problem, and the launch refuses it (rows beyond the scalar kernel's grid, K % 4 != 0)"""
    M, N, K = 65535 * 64 + 1, 9, 3
    a, w = torch.zeros(M, K, device="cuda"), torch.zeros(N, K, device="cuda")
    assert ops.sgemm_route(a, w) == 0 and ops.sgemm_route_shape(M - 1, N, K) == sc.ROUTE_NT
    with pytest.raises(LdtHipError):
        ops.sgemm(a, w)


def test_zz_margins():
    """Not a check: prints the worst err / tol per route and activation (the numbers DESIGN.md section 4.11 quotes)."""
    for k in sorted(RATIOS):
        print("worst err / tol, %-52s %.3f" % (k + ":", RATIOS[k]))
