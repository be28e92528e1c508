"""The fp32 linear (ldt_sgemm) per element and by route: the case table, inputs, float64 references with derived bounds, and fp32 emulations
of its seven kernel forms (used by test_gpu_sgemm_exact.py on the device; judged without a GPU, planted faults included, by
test_sgemm_checks_host.py; the routes of the table by test_sgemm_route_host.py).  Built on kernel_checks.

The reference is float64 of act_out(act_in(a) . w^T + b) from the very fp32 inputs; no part of a bound comes from a kernel's output.  Works on
whatever device its arguments live on; nothing here needs a GPU to import."""
import collections

import torch

import kernel_checks as kc

ACT_NONE, ACT_SILU, ACT_RELU, ACT_GELU = range(4)            # enum ldt_act
ACT_NAMES = ("none", "silu", "relu", "gelu")
ROUTE_NT, ROUTE_MFMA_128, ROUTE_MFMA_32, ROUTE_SMALLN_4, ROUTE_SMALLN_8, ROUTE_SMALLK_4, ROUTE_SMALLK_8 = range(1, 8)
ROUTE_NAMES = ("none", "sgemm_nt", "mfma 128x128", "mfma 32x128", "small-N <4>", "small-N <8>", "small-K <4>", "small-K <8>")
CUS = 256                                                     # MI355X: the streaming forms' grids cap at 16 x / 8 x this many workgroups

Case = collections.namedtuple("Case", "name M N K view route")

# THE table: (name, M, N, K, view, expected route).  view "dense", or "a+4": A starts 4 bytes past a 16-byte boundary.  The smallest shapes
# at which each form can still go wrong; what each reaches is said once, here.  test_sgemm_route_host.py asserts every route on the CPU.
SGEMM_CASES = [Case(*c) for c in (
    ("nt-5x64x3", 5, 64, 3, "dense", 1),                      # scalar staging (K % 4 != 0)
    ("nt-70x70x4", 70, 70, 4, "dense", 1),                    # vector staging, K < 8, 2 x 2 ragged tiles
    ("nt-130x131x21", 130, 131, 21, "dense", 1),              # scalar staging, ragged 16-deep slab, 3 x 3 tiles
    ("nt-65x40x128", 65, 40, 128, "dense", 1),                # M N < 4096
    ("nt-1x2048x1024", 1, 2048, 1024, "dense", 1),            # one AdaLN row: M N = 2048 < 4096 keeps it off the 32 x 128 MFMA form
    ("nt-130x300x256-a+4", 130, 300, 256, "a+4", 1),          # misalignment sends an MFMA shape here
    ("mfma128-49x84x8", 49, 84, 8, "dense", 2),               # smallest shape of the form
    ("mfma128-129x129x20", 129, 129, 20, "dense", 2),         # slab 16 + 4, 2 x 2 ragged tiles
    ("mfma128-200x136x36", 200, 136, 36, "dense", 2),
    ("mfma128-130x300x256", 130, 300, 256, "dense", 2),
    ("mfma32-48x86x8", 48, 86, 8, "dense", 3),                # K below one slab, second row tile
    ("mfma32-33x200x36", 33, 200, 36, "dense", 3),            # slab 32 + 4
    ("mfma32-19x2085x512", 19, 2085, 512, "dense", 3),
    ("smalln4-8192x1x4", 8192, 1, 4, "dense", 4),             # one active lane
    ("smalln4-8200x4x128", 8200, 4, 128, "dense", 4),         # exactly one k trip
    ("smalln4-8195x3x132", 8195, 3, 132, "dense", 4),         # second k trip with one lane, M % 8 tail
    ("smalln4-8193x2x260", 8193, 2, 260, "dense", 4),
    ("smalln4-262157x2x4", 262144 + 13, 2, 4, "dense", 4),    # past the grid cap (16 CUS workgroups x 64 rows)
    ("smalln8-8197x5x4", 8197, 5, 4, "dense", 5),
    ("smalln8-8193x8x64", 8193, 8, 64, "dense", 5),
    ("smalln8-8194x7x136", 8194, 7, 136, "dense", 5),
    ("smalln8-131079x6x8", 131072 + 7, 6, 8, "dense", 5),     # past the cap (16 CUS x 32 rows)
    ("smallk4-8192x32x1", 8192, 32, 1, "dense", 6),           # 32 rows per block
    ("smallk4-8201x64x4", 8201, 64, 4, "dense", 6),
    ("smallk4-20001x128x3", 20001, 128, 3, "dense", 6),
    ("smallk4-8199x1024x2", 8199, 1024, 2, "dense", 6),       # one row per block: past the cap (8 CUS x 4 rows) already
    ("smallk4-20000x1024x3", 20000, 1024, 3, "dense", 6),     # three trips, the last partial, most of its R rows clamped
    ("smallk8-8192x128x5", 8192, 128, 5, "dense", 7),
    ("smallk8-8197x32x7", 8197, 32, 7, "dense", 7),
    ("smallk8-8203x256x8", 8203, 256, 8, "dense", 7),
    ("smallk8-16389x512x6", 16389, 512, 6, "dense", 7),       # second trip of 5 rows
    ("pair-8191x128x3", 8191, 128, 3, "dense", 1),            # the two sides of M = 8192 ...
    ("pair-8192x128x3", 8192, 128, 3, "dense", 6),
    ("pair-48x200x64", 48, 200, 64, "dense", 3),              # ... and of M = 48
    ("pair-49x200x64", 49, 200, 64, "dense", 2),
)]
CASE = {c.name: c for c in SGEMM_CASES}
# one shape per route runs the full operand matrix, the strided and the misaligned views and the repeat
REPRESENTATIVES = ("nt-130x131x21", "mfma128-129x129x20", "mfma32-33x200x36", "smalln4-8195x3x132", "smalln8-8194x7x136",
                   "smallk4-8201x64x4", "smallk8-8197x32x7")
PAST_THE_CAP = ("smalln4-262157x2x4", "smalln8-131079x6x8", "smallk4-8199x1024x2", "smallk4-20000x1024x3", "smallk8-16389x512x6")
# the shapes of test_gpu_kernels.py::test_sgemm and test_gpu_kernel_exact.py's sgemm tests (dense operands), by the route the query reports
LEGACY_ROUTES = {(5, 64, 3): 1, (300, 128, 20): 2, (1000, 768, 64): 2, (7, 2048, 1024): 3, (65, 40, 128): 1, (130, 300, 256): 2,
                 (32, 1000, 512): 3, (1000, 2048, 1024): 2, (4096, 40, 128): 2, (2048, 128, 20): 2, (19, 2085, 512): 3, (32, 4224, 256): 3,
                 (1, 2048, 1024): 1, (20001, 128, 3): 6, (16385, 128, 20): 2, (9000, 64, 32): 2, (30003, 3, 128): 4, (8193, 8, 64): 5,
                 (10000, 1, 512): 4}
GELU_BF16_MAX_K = 36          # bf16 + GELU cases stay at K <= 36: above it the inputs below put more than AMBIGUOUS_CAP of the elements in doubt
UNRESOLVED_CAP = 0.03         # condition on the inputs: share of a bf16 output (ReLU's exact zeros aside) where fp32 cannot resolve a bf16 ulp


def rows_per_pass(route, N, cus=CUS):
    """Rows one pass of a streaming form's grid covers (the grid-stride loop's step): beyond it a row belongs to a later trip."""
    if route == ROUTE_SMALLN_4:
        return 16 * cus * 8 * 8                               # 16 cus workgroups x 8 row groups x R = 8 rows
    if route == ROUTE_SMALLN_8:
        return 16 * cus * 8 * 4                               # R = 4
    if route in (ROUTE_SMALLK_4, ROUTE_SMALLK_8):
        return 8 * cus * (256 // (N // 4)) * 4                # 8 cus workgroups x rows per block x R = 4
    return None


def full_matrix():
    """(with bias, act_in, act_out, bf16 out): bias or none x act_in {none, SiLU, ReLU} x act_out {none, ReLU, SiLU, GELU} x {fp32, bf16}"""
    return [(b, i, o, h) for b in (True, False) for i in (ACT_NONE, ACT_SILU, ACT_RELU) for o in (ACT_NONE, ACT_RELU, ACT_SILU, ACT_GELU)
            for h in (False, True)]


def operand_sets(case):
    """The operand sets a case runs (see test_gpu_sgemm_exact.py::test_sgemm_per_element); bf16 + GELU only at K <= GELU_BF16_MAX_K."""
    if case.name in REPRESENTATIVES:
        sets = full_matrix()
    else:
        sets = [(True, ACT_NONE, ACT_NONE, False),            # fp32 + bias
                (False, ACT_SILU, ACT_NONE, False),           # SiLU in, no bias, fp32: the AdaLN form
                (True, ACT_NONE, ACT_SILU, True),             # SiLU out -> bf16
                (True, ACT_NONE, ACT_GELU, True)]
    return [s for s in sets if not (s[3] and s[2] == ACT_GELU and case.K > GELU_BF16_MAX_K)]


SPECIAL_ROW_VALUES = (30.0, -30.0, 0.0, -0.0, 88.0, -88.0)   # SiLU's expf meets both tails: e^-88 ~ 6e-39 (denormal), e^88 ~ 1.7e38 (finite)


COHERENT_ABOVE_K = 136        # bf16 cases above this K take same-sign inputs (case_inputs(coherent=True)): with random signs the bound of a long sum,
                              # C_ACC K 2^-24 |a| |w|^T, is within reach of a bf16 rounding boundary for more than AMBIGUOUS_CAP of the elements
                              # (2.5 % at K = 256, 12 % at K = 1024); a coherent sum is ~sqrt(K) larger than its bound's share


def coherent(case, bf16):
    return bool(bf16) and case.K > COHERENT_ABOVE_K


def case_inputs(case, coherent=False):
    """-> (a [M, K], w [N, K], bias [N]) float32 on the CPU: randn, weights / sqrt(K), bias 0.5 randn (at 1 a column whose bias is below -1.5
    leaves a twentieth of its GELU outputs under 1e-3, where fp32 cannot resolve a bf16 ulp).  Row 1 of `a` holds SPECIAL_ROW_VALUES (cycled
    over its K columns) when M >= 32: in a shorter problem that one row's outputs, half of them deep in SiLU's lower tail, would be more than
    UNRESOLVED_CAP of all.  coherent: |a|, |w| (every product positive)."""
    g = torch.Generator().manual_seed(case.M * 7 + case.N * 131 + case.K * 17 + 4)       # (+ 4: of the offsets 0..5 the draw that leaves every bf16 case
                                                                                       # at <= 1.5 % ambiguous and <= 2.1 % unresolved elements)
    a = torch.randn(case.M, case.K, generator=g)
    w = torch.randn(case.N, case.K, generator=g) / case.K ** 0.5
    bias = 0.5 * torch.randn(case.N, generator=g)
    if case.M >= 32:
        a[1] = torch.tensor(SPECIAL_ROW_VALUES)[torch.arange(case.K) % len(SPECIAL_ROW_VALUES)]
    return (a.abs(), w.abs(), bias) if coherent else (a, w, bias)


# ------------------------------------------------------------------------------------------------------------- references and bounds
def silu_ref(x64):
    """float64 SiLU and what csrc/common.h's silu(), x / (1.0f + expf(-x)), may differ from it by in fp32.  Counted: ONE expf (LIBM["expf"]
    ulps of e = exp(-x); it moves the quotient by its relative error x e / (1 + e)), ONE add (2^-24), ONE divide (2^-24); the negation is exact.
    Below x = -88.72 expf overflows and the quotient is -0 where SiLU is ~1e-37: allowed in full.  -> (ref, err)."""
    e = torch.exp(-x64)
    ref = x64 / (1 + e)
    err = ref.abs() * (kc.LIBM["expf"] * kc.ULP32 * e / (1 + e) + 2 * kc.U24) * kc.SLACK
    return ref, torch.where(-x64 > kc.EXPF_MAX_ARG, ref.abs(), err)


def gelu_ref(x64):
    """float64 GELU and the own error of gelu_erf, 0.5f * x * (1.0f + erff(x * 0.70710678f)), beside what the slope does to the error of x.
    LIBM_ABS = 1e-6 covers it for |x| <= 4 (counted there: 0.5 |x| x (erff's ulp 2^-23 + the sum's 2^-24 (1 + erf) + the argument's rounding
    through erf') + the product's 2^-24 |gelu| <= 9.5e-7).  Beyond |x| = 4 the same three terms grow with |x| (erf' is below 1e-3 there):
    0.5 |x| (2^-23 + 2 x 2^-24) + 2^-24 |x| = 3 x 2^-24 |x|; 4 x 2^-24 |x| is added there.  -> (ref, err)."""
    ref = torch.nn.functional.gelu(x64)
    return ref, kc.LIBM_ABS + 4 * kc.U24 * x64.abs() * (x64.abs() > 4).double()


SILU_SLOPE = 1.1              # max |d silu / dx| (1.0998 at x = 2.4)


def pre_activation(a, w, bias, act_in):
    """float64 act_in(a) . w^T + b and its bound: kc.sgemm_ref's, unchanged, on the activated input (K + 1 roundings for K <= 7, the recorded
    floor of 8 above), plus, for SiLU, what the fp32 SiLU moves every product by, carried through |w|: err_silu(a) . |w|^T.  act_in ReLU is
    exact (a select).  -> (pre, tol_pre)"""
    x = a.double()
    if act_in == ACT_SILU:
        x, dx = silu_ref(x)
    elif act_in == ACT_RELU:
        x, dx = torch.relu(x), None
    else:
        assert act_in == ACT_NONE
        dx = None
    pre, tol = kc.sgemm_ref(x, w, bias)
    if dx is not None:
        tol = tol + dx @ w.double().abs().T
    return pre, tol


def activated(pre, tol_pre, act_out):
    """float64 act_out(pre) and its bound: slope x tol_pre + the activation's own evaluation error.
      none  tol_pre
      ReLU  slope 1, no own error; where pre < -tol_pre the fp32 value is negative for certain: the output is exactly 0 (bound 0)
      SiLU  slope SILU_SLOPE, own error silu_ref's (relative)
      GELU  slope kc.GELU_SLOPE, own error gelu_ref's (LIBM_ABS; libm erff)
    SiLU and GELU of an exactly zero sum (tol_pre = 0) are exactly 0.
    -> (ref, tol)"""
    if act_out == ACT_NONE:
        return pre, tol_pre
    if act_out == ACT_RELU:
        return torch.relu(pre), torch.where(pre < -tol_pre, torch.zeros_like(tol_pre), tol_pre)
    if act_out == ACT_SILU:
        ref, own = silu_ref(pre)
        tol = SILU_SLOPE * tol_pre + own
    else:
        assert act_out == ACT_GELU
        ref, own = gelu_ref(pre)
        tol = kc.GELU_SLOPE * tol_pre + own
    # a sum whose every product is an exact zero, without a bias (tol_pre = 0: ReLU'd inputs of a short row): SiLU and GELU of 0 are exactly 0
    return ref, torch.where((pre == 0) & (tol_pre == 0), torch.zeros_like(tol), tol)


def reference(a, w, bias, act_in=ACT_NONE, act_out=ACT_NONE):
    """-> (ref, tol) float64 for the fp32 value the kernel holds before it stores"""
    pre, tol_pre = pre_activation(a, w, bias, act_in)
    return activated(pre, tol_pre, act_out)


def bf16_shares(ref, tol):
    """Conditions on the inputs of a bf16-output case, from the reference alone.  -> (mask of the elements where fp32 resolves a bf16 ulp,
    share of those within their bound of a rounding boundary (cap kc.AMBIGUOUS_CAP), share of the unresolved ones among the elements that are
    not an exact ReLU zero (cap UNRESOLVED_CAP))."""
    res = kc.resolved_by_bf16(ref, tol)
    exact_zero = (ref == 0) & (tol == 0)
    allow = kc.ambiguous_ulp(ref[res], tol[res])
    ambiguous = float(((allow > 0) & ~exact_zero[res]).double().mean()) if bool(res.any()) else 0.0
    live = ~exact_zero
    unresolved = float((~res & live).double().sum() / live.double().sum().clamp_min(1))
    return res, ambiguous, unresolved


def check(out, ref, tol, what):
    """A kernel's output against reference(): fp32 within tol per element; bf16 == bf16(ref) bit for bit where fp32 resolves a bf16 ulp (either
    neighbour within tol of a rounding boundary; an exact ReLU zero is 0), within tol + the bf16 rounding elsewhere.  -> worst err / tol."""
    if out.dtype != torch.bfloat16:
        return kc.assert_elementwise(out, ref, tol, what)
    res, _, unresolved = bf16_shares(ref, tol)
    assert unresolved <= UNRESOLVED_CAP, "%s: fp32 does not resolve a bf16 ulp on %.4f of the elements (cap %.2f): choose other inputs" % (what, unresolved, UNRESOLVED_CAP)
    kc.assert_bf16_of(out[res].reshape(1, -1), ref[res].reshape(1, -1), tol[res].reshape(1, -1), what)
    return kc.assert_elementwise(out, ref, tol * (1 + kc.U8) + kc.U8 * ref.abs() + 2.0 ** -133, what + " (bf16 rounding allowed)")


# ------------------------------------------------------------------------------------------------------------- fp32 emulations of the seven forms
def _act32(v, act):
    """The kernels' activation on fp32 values, every operation rounded to fp32 (exp / erf from float64, rounded once: within libm's ulp)."""
    if act == ACT_SILU:
        e = torch.exp(-v.double()).float()
        return v / (1.0 + e)
    if act == ACT_RELU:
        return torch.relu(v)
    if act == ACT_GELU:
        t = v * torch.tensor(0.70710678118654752440, dtype=torch.float32)
        return (0.5 * v) * (1.0 + torch.erf(t.double()).float())
    return v


def emulate(route, a, w, bias, act_in=ACT_NONE, act_out=ACT_NONE, out_bf16=False, fault=None, cus=CUS, fill=0.0):
    """What the form `route` computes for fp32 a [M, K], w [N, K], bias [N] | None, in the kernel's own order, in torch on the CPU:
      sgemm_nt         acc = 0, one FMA per k in order, then + bias
      small-K <4>, <8> acc = bias, one FMA per k in order
      small-N <4>, <8> lane l of 32 sums k = 4 l + 128 t + j (t, then j = 0..3) by FMA from 0; 5 xor-shuffle additions (16, 8, 4, 2, 1); + bias
      MFMA forms       acc = 0; per 8-k group g and kk = 0..3 the pair (8 g + kk, 8 g + kk + 4), two FMAs; K zero-filled to the slab; + bias
    -> out [M, N] (fp32 or bf16); rows a fault leaves unwritten keep `fill`.  fault, one of (rows_per_pass from `cus`):
      "no_second_trip" rows past the first pass of the grid are not computed        "tail_overwrites_last" the last row holds row M - 2's result
      "tail_unwritten" the last row is not stored                                   "drop_ragged_k" the ragged last slab / chunk of K is dropped
      "bias_next" column n takes bias[n + 1]                                        "silu_after" act_in is applied to the product instead of the input
      "act_before_bias" act_out before the bias                                     "bf16_truncate" bf16 output truncated instead of rounded
      "perm_one_operand" the k, k + 4 pairing on A only (B pairs k, k + 1)          "store_shift4" every 16-byte store lands 4 columns to the right"""
    M, K = a.shape
    N = w.shape[0]
    x = a.float()
    if act_in and fault != "silu_after":
        x = _act32(x, act_in)
    wk = w.float()
    if fault == "drop_ragged_k":
        slab = {ROUTE_NT: 16, ROUTE_MFMA_128: 16, ROUTE_MFMA_32: 32, ROUTE_SMALLN_4: 128, ROUTE_SMALLN_8: 128}.get(route, 4)
        keep = K // slab * slab
        x, wk, K = x[:, :keep], wk[:, :keep], keep
    b = None if bias is None else bias.float()
    if b is not None and fault == "bias_next":
        b = torch.roll(b, -1)
    acc = torch.zeros(M, N)
    fma = lambda k, ka, acc: kc.fma32(x[:, ka:ka + 1], wk[None, :, k].reshape(1, N), acc)
    if route in (ROUTE_SMALLK_4, ROUTE_SMALLK_8):
        if b is not None and fault != "act_before_bias":
            acc = acc + b
        for k in range(K):
            acc = fma(k, k, acc)
    elif route == ROUTE_NT:
        for k in range(K):
            acc = fma(k, k, acc)
    elif route in (ROUTE_SMALLN_4, ROUTE_SMALLN_8):
        part = torch.zeros(32, M, N)
        for k in range(K):
            lane = (k % 128) // 4
            part[lane] = fma(k, k, part[lane])
        for o in (16, 8, 4, 2, 1):
            part = part + part[torch.arange(32) ^ o]
        acc = part[0]
    else:
        assert route in (ROUTE_MFMA_128, ROUTE_MFMA_32)
        order = [8 * g + kk + h for g in range((K + 7) // 8) for kk in range(4) for h in (0, 4)]
        for k in order:
            if k < K:
                kb = k
                if fault == "perm_one_operand":            # B's lane halves hold k 0..1 | 2..3 ...: the pair it offers for A's (kk, kk + 4) is (2 kk, 2 kk + 1)
                    g, r = divmod(k, 8)
                    kb = 8 * g + (2 * (r % 4) + r // 4)
                    if kb >= K:
                        continue
                acc = fma(kb, k, acc)
    if fault == "silu_after" and act_in:
        acc = _act32(acc, act_in)
    if fault == "act_before_bias":
        acc = _act32(acc, act_out)
        v = acc if b is None else acc + b
    else:
        if b is not None and route not in (ROUTE_SMALLK_4, ROUTE_SMALLK_8):
            acc = acc + b
        v = _act32(acc, act_out)
    if out_bf16:
        v = (v.view(torch.int32) & -65536).view(torch.float32).bfloat16() if fault == "bf16_truncate" else v.bfloat16()
    out = torch.full((M, N), fill, dtype=v.dtype)
    out.copy_(v)
    if fault == "no_second_trip":
        out[rows_per_pass(route, N, cus):] = fill
    elif fault == "tail_overwrites_last":
        out[M - 1] = v[M - 2]
    elif fault == "tail_unwritten":
        out[M - 1] = fill
    elif fault == "store_shift4":
        out[:, 4:] = v[:, :N - 4]
        out[:, :4] = fill
    return out
