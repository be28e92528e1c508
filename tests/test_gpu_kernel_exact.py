"""GPU (-m gpu): per-element bounds and exact probes on every MFMA kernel route (helpers: tests/kernel_checks.py).

test_gpu_kernels.py judges bf16 outputs by one global rel-MSE, which a few hundred entirely wrong elements of a 67 M element output pass.
Here every default-reachable GEMM form (ROUTES: pinned to what ops.gemm_route reports, asserted before every launch) and every attention
route is held (a) to a componentwise bound against float64 on randn data, (b) to torch.equal on operands whose result is exact in any
summation order (one-hot selection, small integers, a softmax that gathers one key), and (c) to bit-equality with the dense call when
operands and outputs are interiors of larger buffers whose surround is NaN / a sentinel that must survive."""
import collections

import pytest
import torch

import kernel_checks as kc
import sgemm_checks as sc

pytestmark = pytest.mark.gpu

ops = None
EPI = {}
RATIOS = collections.defaultdict(float)          # worst err / tol per class of check (printed by test_zz_margins)


@pytest.fixture(scope="module", autouse=True)
def _mods():
    global ops
    assert torch.cuda.is_available()
    from ldt_amd import _lib, ops as _ops
    ops = _ops
    EPI.update(F32=_lib.EPI_F32, BF16=_lib.EPI_BF16, GELU=_lib.EPI_GELU_BF16, RELU=_lib.EPI_RELU_BF16, RESID=_lib.EPI_RESID_F32)
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    _CACHE.clear()


def dev(x, dt=None):
    return x.to("cuda", dt) if dt else x.to("cuda")


def note(kind, ratio):
    RATIOS[kind] = max(RATIOS[kind], ratio)
    return ratio


# ------------------------------------------------------------------------------------------------------------- route table
ALL = ("F32", "BF16", "GELU", "RELU", "RESID")
MID = ("F32", "BF16", "GELU", "RESID")             # (the mid-size tile kernel has no ReLU form: those go to v1)
ROUTES = []


def _rows(tag, epis, M, N, K, expected, fold=0):
    for e in epis:
        ROUTES.append(pytest.param(e, M, N, K, fold, expected, id="%s-%s-%dx%dx%d%s" % (tag, e.lower(), M, N, K, "-g%d" % fold if fold else "")))


# expectations derived once from ops.gemm_route and pinned: (family, BM, BN, tiles per workgroup).  A retuned launcher fails HERE, with
# "this shape no longer tests the kernel it was chosen for", instead of silently leaving a tile form untested.
_rows("one", ALL, 16384, 1024, 1024, ("256-one-tile", 256, 256, 1))
_rows("one", ("BF16", "RESID"), 16384, 1024, 4096, ("256-one-tile", 256, 256, 1))
_rows("multi", ALL, 16384, 4096, 1024, ("256-multi-tile", 256, 256, 4))
_rows("multi", ("F32", "BF16"), 16384, 3072, 1024, ("256-multi-tile", 256, 256, 3))
_rows("multi", ("GELU", "RESID"), 66560, 256, 256, ("256-multi-tile", 256, 256, 2))       # 260 tiles: four workgroups take a second one
# grid == tiles, yet the kernels' tile list hands one workgroup two tiles (164 tiles, no multiple of 8): the multi-tile form must run
_rows("multi", ("RESID", "BF16"), 10496, 1024, 1024, ("256-multi-tile", 256, 256, 2))
_rows("multi", ("RESID",), 10496, 1024, 4096, ("256-multi-tile", 256, 256, 2))
for _K in (64, 128, 192, 256):                     # 3-stage ring: 1, 2, stages, stages + 1 K-tiles
    _rows("mid", MID, 2048, 4096, _K, ("mid", 128, 256, 1))
    _rows("mid", ("BF16", "GELU"), 2048, 3072, _K, ("mid", 128, 192, 1))
    _rows("mid", MID, 1024, 4096, _K, ("mid", 128, 128, 1))
_rows("mid", MID, 1960, 4096, 320, ("mid", 128, 256, 1))                                  # ragged last row tile
_rows("mid", ("BF16", "GELU"), 1990, 3072, 320, ("mid", 128, 192, 1))
_rows("mid", MID, 1000, 2304, 320, ("mid", 128, 128, 1))
for _K in (64, 128, 256, 320):                     # 4-stage ring
    _rows("mid", MID, 2048, 1024, _K, ("mid", 64, 128, 1))
_rows("mid", MID, 2000, 1024, 192, ("mid", 64, 128, 1))
for _K in (64, 128, 384, 448):                     # 6-stage ring
    _rows("mid", MID, 1024, 1024, _K, ("mid", 64, 64, 1))
_rows("mid", MID, 1000, 1024, 704, ("mid", 64, 64, 1))
_rows("v1", ALL, 5000, 1720, 64, ("v1", 128, 128, 1))                                     # ragged M and N
_rows("v1", ALL, 5000, 840, 128, ("v1", 128, 64, 1))
_rows("v1", ALL, 130, 132, 64, ("v1", 64, 64, 1))
_rows("v1", ALL, 77, 64, 192, ("v1", 64, 64, 1))
_rows("v1", ("RELU",), 2048, 4096, 128, ("v1", 128, 128, 1))
# LN-folded forms: producer (RESID) and consumers (BF16 / GELU), statistics per 256 columns (256-tile kernel) and per 32 (mid-size tile kernel)
_rows("fold", ("RESID",), 512, 1024, 512, ("256-one-tile", 256, 256, 1), 256)
_rows("fold", ("BF16",), 512, 768, 1024, ("256-one-tile", 256, 256, 1), 256)
_rows("fold", ("RESID", "GELU"), 66560, 256, 256, ("256-multi-tile", 256, 256, 2), 256)
_rows("fold", ("RESID",), 768, 768, 256, ("256-multi-tile", 256, 256, 2), 256)               # 9 tiles on 9 workgroups: the smallest such launch
_rows("fold", ("RESID",), 16384, 1024, 1024, ("256-one-tile", 256, 256, 1), 256)
_rows("fold", ("GELU",), 16384, 4096, 1024, ("256-multi-tile", 256, 256, 4), 256)         # MLP-up + GELU: the largest share of a step
_rows("fold", ("BF16",), 16384, 3072, 1024, ("256-multi-tile", 256, 256, 3), 256)
_rows("fold", ("RESID",), 2048, 1024, 512, ("mid", 64, 128, 1), 32)
_rows("fold", ("RESID",), 4096, 1024, 512, ("mid", 128, 128, 1), 32)
_rows("fold", ("BF16",), 2048, 3072, 1024, ("mid", 128, 192, 1), 32)
_rows("fold", ("GELU",), 2048, 4096, 1024, ("mid", 128, 256, 1), 32)
_rows("fold", ("BF16",), 1024, 1024, 1024, ("mid", 128, 128, 1), 32)


def check_route(epi, M, N, K, fold, expected):
    got = tuple(ops.gemm_route(EPI[epi], M, N, K, fold=fold))
    assert got == expected, ("%s %dx%dx%d (fold %d) now runs %r: this shape no longer tests the kernel it was chosen for, %r"
                             % (epi, M, N, K, fold, got, expected))


@pytest.mark.parametrize("epi,M,N,K,fold,expected", ROUTES)
def test_route_table(epi, M, N, K, fold, expected):
    check_route(epi, M, N, K, fold, expected)


def test_route_table_reaches_every_default_form():
    forms = {(p.values[4],) + p.values[5][:3] for p in ROUTES}
    want = {(0, "256-one-tile", 256, 256), (0, "256-multi-tile", 256, 256), (256, "256-one-tile", 256, 256), (256, "256-multi-tile", 256, 256)}
    want |= {(0, "mid", bm, bn) for bm, bn in ((128, 256), (128, 192), (128, 128), (64, 128), (64, 64))}
    want |= {(32, "mid", bm, bn) for bm, bn in ((128, 256), (128, 192), (128, 128), (64, 128))}
    want |= {(0, "v1", bm, bn) for bm, bn in ((128, 128), (128, 64), (64, 64))}
    assert forms == want, forms ^ want
    # what the query reports for problems no kernel takes, and that a workgroup cap moves the 5/8 rule as the launcher's does
    assert ops.gemm_route(EPI["BF16"], 256, 256, 72).family == "none"
    assert ops.gemm_route(EPI["RESID"], 2048, 1024, 512, fold=32).family == "mid" and ops.gemm_route(EPI["RELU"], 2048, 1024, 512, fold=32).family == "none"
    assert tuple(ops.gemm_route(EPI["BF16"], 8192, 1024, 1024, max_wgs=128)) == ("256-one-tile", 256, 256, 1)
    assert ops.gemm_route(EPI["BF16"], 8192, 1024, 1024).family == "mid"


# ------------------------------------------------------------------------------------------------------------- operands + float64 references
_CACHE = {}


def on_device_ref(M, N, K):
    return M * N * K >= 1 << 30                     # large rows: float64 matmul on the device (an independent library); small ones on the CPU


def mm64(x, w, big):
    """float64 x @ w^T (x, w float32 CPU tensors) -> device float64."""
    if big:
        return dev(x).double() @ dev(w).double().T
    return dev(x.double() @ w.double().T)


def randn_problem(M, N, K):
    """-> dict(x, w, bias on the CPU (bf16-exact float32 / float32), xd, wd, bd on the device, pre = float64 x w^T + bias and acc =
    gemm_acc_err on the device); the last problem is kept so that the epilogues of one shape share it."""
    key = ("randn", M, N, K)
    if key not in _CACHE:
        _CACHE.clear()
        torch.cuda.empty_cache()
        g = torch.Generator().manual_seed(M * 3 + N * 5 + K)
        x = torch.randn(M, K, generator=g).bfloat16().float()
        w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().float()
        bias = torch.randn(N, generator=g)
        big = on_device_ref(M, N, K)
        pre = mm64(x, w, big) + dev(bias).double()
        acc = mm64(x.abs(), w.abs(), big) + dev(bias).double().abs()
        _CACHE[key] = dict(x=x, w=w, bias=bias, xd=dev(x, torch.bfloat16), wd=dev(w, torch.bfloat16), bd=dev(bias), pre=pre, absacc=acc, g=g)
    return _CACHE[key]


def test_device_float64_reference_matches_cpu():
    """The device float64 matmul that serves as the reference of the large rows, against CPU float64 on 64 sampled rows."""
    M, N, K = 16384, 1024, 4096
    p = randn_problem(M, N, K)
    rows = torch.arange(64) * 251 + 7
    cpu = p["x"][rows].double() @ p["w"].double().T + p["bias"].double()
    got = p["pre"][dev(rows)].cpu()
    assert float((got - cpu).abs().max()) <= 1e-12 * float(cpu.abs().max())


def acc_err(p, K):
    return p["absacc"] * (kc.C_ACC * K * kc.U24)


# ------------------------------------------------------------------------------------------------------------- bound vs float64, randn data
def _plain_bound(epi, M, N, K):
    p = randn_problem(M, N, K)
    xd, wd, bd, pre, g = p["xd"], p["wd"], p["bd"], p["pre"], p["g"]
    acc = acc_err(p, K)
    what = "%s %dx%dx%d" % (epi, M, N, K)
    if epi == "F32":
        r = kc.assert_elementwise(ops.gemm_bf16(xd, wd, bd, EPI["F32"]), pre, acc + kc.U24 * pre.abs(), what)
        return note("gemm fp32 out", r)
    if epi == "BF16":
        return note("gemm bf16 out", kc.assert_elementwise(ops.gemm_bf16(xd, wd, bd, EPI["BF16"]), pre, acc * (1 + kc.U8) + kc.U8 * pre.abs(), what))
    if epi == "GELU":
        ref = torch.nn.functional.gelu(pre)
        tol = (acc * kc.GELU_SLOPE + kc.GELU_FAST_ABS) * (1 + kc.U8) + kc.U8 * ref.abs()
        return note("gemm gelu bf16 out", kc.assert_elementwise(ops.gemm_bf16(xd, wd, bd, EPI["GELU"]), ref, tol, what))
    if epi == "RELU":
        skip = torch.randn(M, N, generator=g).bfloat16()
        sd = dev(skip)
        ref = torch.relu(pre + sd.double())
        tol = (acc + kc.U24 * (pre.abs() + sd.double().abs())) * (1 + kc.U8) + kc.U8 * ref.abs()
        r = kc.assert_elementwise(ops.gemm_bf16(xd, wd, bd, EPI["RELU"], skip=sd), ref, tol, what + " + skip")
        ref = torch.relu(pre)
        r = max(r, kc.assert_elementwise(ops.gemm_bf16(xd, wd, bd, EPI["RELU"]), ref, acc * (1 + kc.U8) + kc.U8 * ref.abs(), what))
        return note("gemm relu bf16 out", r)
    assert epi == "RESID"
    resid = dev(torch.randn(M, N, generator=g))
    worst = 0.0
    rps = 8 if M % 8 == 0 else M
    gate = dev(torch.randn(M // rps, 3 * N, generator=g))
    gates = dev(torch.randn(3, 2 * N, generator=g))
    step = torch.tensor([2], dtype=torch.int32, device="cuda")
    for label, kw, gfull in (
            ("per-sample gate", dict(gate=gate[:, N:2 * N], gate_sample_stride=3 * N, rows_per_sample=rps), gate[:, N:2 * N].double().repeat_interleave(rps, 0)),
            ("step-indexed shared gate", dict(gate=gates[:, N:], gate_sample_stride=0, rows_per_sample=M, step_ptr=step, gate_step_stride=2 * N), gates[2, N:].double()),
            ("no gate", {}, None)):
        rd = resid.clone()
        ops.gemm_bf16(xd, wd, bd, EPI["RESID"], out=rd, resid=rd, **kw)
        upd = pre if gfull is None else gfull * pre
        ref = resid.double() + upd
        tol = (acc if gfull is None else gfull.abs() * acc) + 2 * kc.U24 * (resid.double().abs() + upd.abs()) + kc.U24 * ref.abs()
        worst = max(worst, kc.assert_elementwise(rd, ref, tol, "%s, %s" % (what, label)))
    return note("gemm resid fp32 out", worst)


def _fold_problem(M, N, K, granule, seed):
    """Producer operands at (M, N, K): a bf16 [M, K], wo bf16 [N, K], bias, residual stream x0 with a row mean that is not small, gate, ln_scale."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).bfloat16().float()
    wo = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().float()
    bo = torch.randn(N, generator=g)
    x0 = torch.randn(M, N, generator=g) * 1.5 + 0.6
    rps = 128 if M < 4096 else M // 2
    gate = torch.randn(M // rps, N, generator=g)
    sc = 0.3 * torch.randn(N, generator=g)
    return a, wo, bo, x0, rps, gate, sc


def _producer_bound(M, N, K, granule):
    a, wo, bo, x0, rps, gate, sc = _fold_problem(M, N, K, granule, M + N + K)
    big = on_device_ref(M, N, K)
    pre = mm64(a, wo, big) + dev(bo).double()
    acc = (mm64(a.abs(), wo.abs(), big) + dev(bo).double().abs()) * (kc.C_ACC * K * kc.U24)
    gfull = dev(gate).double().repeat_interleave(rps, 0)
    xd = dev(x0.clone())
    xs, stats = ops.gemm_resid_lnstats(dev(a, torch.bfloat16), dev(wo, torch.bfloat16), dev(bo), xd, dev(sc), gate=dev(gate),
                                       gate_sample_stride=N, rows_per_sample=rps, granule=granule)
    what = "LN-fold producer %dx%dx%d granule %d" % (M, N, K, granule)
    x064 = dev(x0).double()
    xref = x064 + gfull * pre
    tol_x = gfull.abs() * acc + 2 * kc.U24 * (x064.abs() + (gfull * pre).abs()) + kc.U24 * xref.abs()
    r = kc.assert_elementwise(xd, xref, tol_x, what + ": x")
    s1 = 1 + dev(sc).double()
    xs_ref = xref * s1
    r = max(r, kc.assert_elementwise(xs, xs_ref, (tol_x * s1.abs() + 2 * kc.U24 * xs_ref.abs()) * (1 + kc.U8) + kc.U8 * xs_ref.abs(), what + ": xs"))
    # the statistics are sums over the fp32 values the kernel stored: compared with float64 sums of ITS x, to fp32 summation round-off
    assert stats.shape == (N // granule, M, 2)
    tiles = xd.double().view(M, N // granule, granule)
    for j, (name, t) in enumerate((("sum", tiles), ("sum of squares", tiles * tiles))):
        want = t.sum(-1).T
        r = max(r, kc.assert_elementwise(stats[..., j], want, granule * kc.U24 * t.abs().sum(-1).T, "%s: row %s per %d columns" % (what, name, granule)))
    return note("LN-fold producer", r)


def _consumer_bound(epi, M, N, K, granule):
    """Consumer alone, on operands given exactly: xs bf16 and the row statistics of x = xs (ln_scale = 0) in fp32.  Reference: the same
    algebra in float64 FROM those fp32 statistics, so the only differences are fp32 accumulation, the fp32 mean / rstd and the bf16 output."""
    g = torch.Generator().manual_seed(M + N + K + granule)
    xs = (torch.randn(M, K, generator=g) * 1.2 + 0.4).bfloat16().float()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().float()
    S = torch.randn(N, generator=g); C = torch.randn(N, generator=g)
    t = dev(xs).double().view(M, K // granule, granule)
    stats = torch.stack([t.sum(-1).T, (t * t).sum(-1).T], -1).float().contiguous()          # [K / granule, M, 2]
    y = ops.gemm_lnfold(dev(xs, torch.bfloat16), dev(w, torch.bfloat16), stats, dev(S), dev(C), EPI[epi])
    s = stats.double().sum(0)
    mean = s[:, 0:1] / K
    rstd = 1 / torch.sqrt((s[:, 1:2] / K - mean * mean).clamp_min(0) + 1e-6)
    big = on_device_ref(M, N, K)
    mm = mm64(xs, w, big)
    t1, t2, t3 = rstd * mm, rstd * mean * dev(S).double(), dev(C).double()
    ref = t1 - t2 + t3
    # fp32 accumulation; mean, variance (a difference of two fp32 terms) and rsqrt in fp32: 2^-19 relative on every term they scale
    acc = rstd * mm64(xs.abs(), w.abs(), big) * (kc.C_ACC * K * kc.U24) + 2.0 ** -19 * (t1.abs() + t2.abs() + t3.abs())
    if epi == "GELU":
        ref = torch.nn.functional.gelu(ref)
        acc = acc * kc.GELU_SLOPE + kc.GELU_FAST_ABS
    r = kc.assert_elementwise(y, ref, acc * (1 + kc.U8) + kc.U8 * ref.abs(), "LN-fold consumer %s %dx%dx%d granule %d" % (epi, M, N, K, granule))
    return note("LN-fold consumer bf16 out", r)


@pytest.mark.parametrize("epi,M,N,K,fold,expected", ROUTES)
def test_gemm_bound_vs_float64(epi, M, N, K, fold, expected):
    check_route(epi, M, N, K, fold, expected)
    if not fold:
        r = _plain_bound(epi, M, N, K)
    elif epi == "RESID":
        r = _producer_bound(M, N, K, fold)
    else:
        r = _consumer_bound(epi, M, N, K, fold)
    print("worst err / tol %.3f (%s %dx%dx%d fold %d -> %s)" % (r, epi, M, N, K, fold, expected[0]))


# ------------------------------------------------------------------------------------------------------------- exact probes
def _exact_plain(epi, M, N, K):
    for probe in ("selection", "integer"):
        key = (probe, M, N, K)
        if key not in _CACHE:
            _CACHE.clear()
            torch.cuda.empty_cache()
            if probe == "selection":
                x, w, ref = kc.selection_probe(M, N, K)
                bias, ref = None, dev(ref).double()
            else:
                x, w, bias, ref = kc.integer_probe(M, N, K, seed=M + N + K, device="cuda")
            _CACHE[key] = (dev(x, torch.bfloat16), dev(w, torch.bfloat16), None if bias is None else dev(bias), ref)
        xd, wd, bd, ref = _CACHE[key]
        what = "%s probe, %s %dx%dx%d" % (probe, epi, M, N, K)
        g = torch.Generator().manual_seed(M + K)
        if epi == "F32":
            kc.assert_elementwise(ops.gemm_bf16(xd, wd, bd, EPI["F32"]), ref, 0.0, what)
        elif epi == "BF16":
            kc.assert_elementwise(ops.gemm_bf16(xd, wd, bd, EPI["BF16"]), ref, 0.0, what)
        elif epi == "RELU":
            kc.assert_elementwise(ops.gemm_bf16(xd, wd, bd, EPI["RELU"]), torch.relu(ref), 0.0, what)
            if probe == "integer":                                      # + a small-integer skip: |ref + skip| stays an integer <= 256 + 3
                skip = dev(torch.randint(-3, 4, (M, N), generator=g).float())
                want = torch.relu(ref + skip.double()).float().bfloat16().double()     # (257..259 round in bf16: the same rounding, stated)
                kc.assert_elementwise(ops.gemm_bf16(xd, wd, bd, EPI["RELU"], skip=skip.bfloat16()), want, 0.0, what + " + skip")
        elif epi == "GELU":
            want = torch.nn.functional.gelu(ref)
            tol = kc.bf16_ulp(want) + kc.GELU_FAST_ABS                  # one bf16 ulp per element
            note("gelu on exact pre-activations (ulp)", kc.assert_elementwise(ops.gemm_bf16(xd, wd, bd, EPI["GELU"]), want, tol, what))
        else:
            # residual and gates small integers: resid + gate * (x w^T + bias) is an integer far below 2^24, exact in fp32 in any order
            resid = dev(torch.randint(-50, 51, (M, N), generator=g).float())
            rps = 8 if M % 8 == 0 else M
            gate = dev(torch.randint(-3, 4, (M // rps, N), generator=g).float())
            rd = resid.clone()
            ops.gemm_bf16(xd, wd, bd, EPI["RESID"], out=rd, resid=rd, gate=gate, gate_sample_stride=N, rows_per_sample=rps)
            kc.assert_elementwise(rd, resid.double() + gate.double().repeat_interleave(rps, 0) * ref, 0.0, what + ", per-sample gate")
            gates = dev(torch.randint(-3, 4, (3, N), generator=g).float())
            step = torch.tensor([1], dtype=torch.int32, device="cuda")
            rd = resid.clone()
            ops.gemm_bf16(xd, wd, bd, EPI["RESID"], out=rd, resid=rd, gate=gates, gate_sample_stride=0, rows_per_sample=M, step_ptr=step, gate_step_stride=N)
            kc.assert_elementwise(rd, resid.double() + gates[1].double() * ref, 0.0, what + ", step-indexed shared gate")
            rd = resid.clone()
            ops.gemm_bf16(xd, wd, bd, EPI["RESID"], out=rd, resid=rd)
            kc.assert_elementwise(rd, resid.double() + ref, 0.0, what + ", no gate")


def _exact_producer(M, N, K, granule):
    """Integer probe through the LN-fold producer with ln_scale in {0, 1} (1 + scale a power of two): x, xs and the statistics exact."""
    x, w, bias, ref = kc.integer_probe(M, N, K, seed=M + N + K + 1, max_abs=100, device="cuda")
    g = torch.Generator().manual_seed(M + N)
    x0 = torch.randint(-20, 21, (M, N), generator=g).float()
    rps = 128 if M < 4096 else M // 2
    gate = (1 - 2 * torch.randint(0, 2, (M // rps, N), generator=g)).float()
    sc = torch.randint(0, 2, (N,), generator=g).float()
    want = dev(x0).double() + dev(gate).double().repeat_interleave(rps, 0) * ref
    tiles = want.view(M, N // granule, granule)
    assert float(want.abs().max()) <= 128 and float((tiles * tiles).sum(-1).max()) < 2 ** 24       # xs <= 256 and every statistic exact in fp32
    xd = dev(x0.clone())
    xs, stats = ops.gemm_resid_lnstats(dev(x, torch.bfloat16), dev(w, torch.bfloat16), dev(bias), xd, dev(sc), gate=dev(gate),
                                       gate_sample_stride=N, rows_per_sample=rps, granule=granule)
    what = "integer probe, LN-fold producer %dx%dx%d granule %d" % (M, N, K, granule)
    kc.assert_elementwise(xd, want, 0.0, what + ": x")
    kc.assert_elementwise(xs, want * (1 + dev(sc).double()), 0.0, what + ": xs")
    kc.assert_elementwise(stats[..., 0], tiles.sum(-1).T, 0.0, what + ": row sums")
    kc.assert_elementwise(stats[..., 1], (tiles * tiles).sum(-1).T, 0.0, what + ": row sums of squares")


@pytest.mark.parametrize("epi,M,N,K,fold,expected", [p for p in ROUTES if not (p.values[4] and p.values[0] != "RESID")])
def test_gemm_exact_probes(epi, M, N, K, fold, expected):
    check_route(epi, M, N, K, fold, expected)
    if fold:
        _exact_producer(M, N, K, fold)
    else:
        _exact_plain(epi, M, N, K)


@pytest.mark.parametrize("M,N,K", [(1000, 768, 64), (130, 300, 256), (1000, 2048, 1024),        # 128 x 128 MFMA
                                   (19, 2085, 512),                                             # 32 x 128 MFMA
                                   (20001, 128, 3), (30003, 3, 128), (10000, 1, 512),           # streaming: small-K <4>, small-N <4>, small-N <4>
                                   (1, 2048, 1024), (5, 64, 3), (65, 40, 128)])                 # scalar-FMA kernel (M N < 4096; K % 4 != 0)
def test_sgemm_selection_probe(M, N, K):
    x, w, ref = kc.selection_probe(M, N, K)
    b = (torch.arange(N) % 7 - 3).float()
    assert ops.sgemm_route(dev(x), dev(w), dev(b)) == sc.LEGACY_ROUTES[(M, N, K)]
    out = ops.sgemm(dev(x), dev(w), dev(b))
    kc.assert_elementwise(out, dev(ref).double() + dev(b).double(), 0.0, "selection probe, sgemm %dx%dx%d" % (M, N, K))


# the route of every shape, by the launcher's own query: sgemm_checks.LEGACY_ROUTES (asserted on the CPU by test_sgemm_route_host.py and below)
SGEMM = [(5, 64, 3), (300, 128, 20), (1000, 768, 64), (7, 2048, 1024), (65, 40, 128), (130, 300, 256), (32, 1000, 512), (1000, 2048, 1024),
         (4096, 40, 128), (2048, 128, 20),                     # scalar-FMA kernel (5 x 64 x 3, 65 x 40 x 128), 32 x 128 MFMA (M = 7, 32), else 128 x 128 MFMA
         (19, 2085, 512), (32, 4224, 256), (1, 2048, 1024),    # 32 x 128 MFMA (M <= 48); M = 1 has M N < 4096: scalar-FMA kernel
         (20001, 128, 3), (16385, 128, 20), (9000, 64, 32),    # M >= 8192: small-K <4>, then two shapes with K > 8 and N > 8: 128 x 128 MFMA
         (30003, 3, 128), (8193, 8, 64), (10000, 1, 512)]      # small-N <4>, <8>, <4>


@pytest.mark.parametrize("M,N,K", SGEMM)
def test_sgemm_bound_and_integer_probe(M, N, K):
    """ops.sgemm on the shapes of test_gpu_kernels.py::test_sgemm (six of the seven kernel forms; all seven, with activations and views:
    test_gpu_sgemm_exact.py), per element: randn data against float64 within the fp32
    accumulation bound, and the integer probe exactly.  The bound's factor on 2^-24 (|a| |w|^T + |b|): K + 1 roundings at the worst; these
    kernels add their products one after another (fp32 FMA chains, 32 x 32 x 2 MFMAs), so their error grows like sqrt(K) with a larger
    constant than the blocked bf16 kernels': measured on the MI355X up to 4.7 at K = 64 and 3.9 at K = 20, hence a floor of 8 under C_ACC K."""
    g = torch.Generator().manual_seed(K * 7 + N)
    a = dev(torch.randn(M, K, generator=g)); w = dev(torch.randn(N, K, generator=g) / K ** 0.5); b = dev(torch.randn(N, generator=g))
    assert ops.sgemm_route(a, w, b) == sc.LEGACY_ROUTES[(M, N, K)]
    ref, tol = kc.sgemm_ref(a, w, b)
    r = kc.assert_elementwise(ops.sgemm(a, w, b), ref, tol, "sgemm %dx%dx%d" % (M, N, K))
    tol_r = tol + kc.U24 * torch.relu(ref)
    r = max(r, kc.assert_elementwise(ops.sgemm(a, w, b, act_out=2), torch.relu(ref), tol_r, "sgemm + ReLU %dx%dx%d" % (M, N, K)))   # ACT_RELU
    print("worst err / tol %.3f (sgemm %dx%dx%d)" % (note("sgemm fp32 out", r), M, N, K))
    x, wi, bias, iref = kc.integer_probe(M, N, K, seed=M + N + K, device="cuda")
    kc.assert_elementwise(ops.sgemm(dev(x), dev(wi), dev(bias)), iref, 0.0, "integer probe, sgemm %dx%dx%d" % (M, N, K))


# ------------------------------------------------------------------------------------------------------------- attention
ATTN = [  # B, H, Nq, Nk, dh, route (0 streaming, 1 resident, 2 whole-head)
    (2, 4, 256, 256, 64, 2), (2, 4, 256, 256, 32, 0), (3, 4, 129, 129, 64, 2), (2, 2, 129, 129, 32, 0), (2, 2, 255, 65, 64, 2), (2, 2, 255, 65, 32, 0),
    (2, 4, 300, 77, 32, 0), (2, 2, 300, 77, 64, 0), (1, 4, 2048, 256, 32, 0), (1, 2, 2048, 256, 64, 0), (2, 4, 40, 2048, 32, 0), (1, 2, 40, 256, 64, 1),
    (2, 2, 8, 5, 32, 1), (2, 2, 8, 5, 64, 1), (2, 2, 128, 512, 32, 1)]


def _route(B, H, Nq, Nk, dh):
    from ldt_amd import _lib
    return int(_lib.lib().ldt_attention_route(B, H, Nq, Nk, dh))


def test_attention_routes_all_reached():
    assert {(r, dh) for *_, dh, r in ATTN} >= {(0, 32), (0, 64), (1, 32), (1, 64), (2, 64)}


@pytest.mark.parametrize("B,H,Nq,Nk,dh,route", ATTN)
def test_attention_gather_probe(B, H, Nq, Nk, dh, route):
    assert _route(B, H, Nq, Nk, dh) == route, "this shape no longer tests the attention kernel it was chosen for"
    q, k, v, want = kc.attention_gather_probe(B, H, Nq, Nk, dh, seed=Nq + Nk)
    C = H * dh
    out = ops.attention_fwd(dev(q, torch.bfloat16).view(B * Nq, C), dev(k, torch.bfloat16).view(B * Nk, C), dev(v, torch.bfloat16).view(B * Nk, C),
                            B, H, Nq, Nk, dh)
    kc.assert_elementwise(out.reshape(B * H * Nq, dh), dev(want).double().reshape(B * H * Nq, dh), 0.0,
                          "gather probe, attention route %d, B %d H %d Nq %d Nk %d Dh %d (row = (b H + h) Nq + query)" % (route, B, H, Nq, Nk, dh))


@pytest.mark.parametrize("B,H,Nq,Nk", [(2, 4, 256, 256), (3, 2, 200, 77), (2, 4, 2048, 256), (2, 2, 40, 2048), (2, 2, 8, 5), (256, 4, 512, 256)])
def test_attention_oproj_gather_probe(B, H, Nq, Nk):
    """The fused attention + output projection + residual kernel with Wo = I, bo = 0, no gate, x = 0: x becomes exactly the [B][H][Nq][Dh]
    gather re-read as (B Nq, C) rows — quirk Q1's row mapping, per element."""
    dh = 32
    C = H * dh
    q, k, v, want = kc.attention_gather_probe(B, H, Nq, Nk, dh, seed=B + Nq + Nk)
    x = torch.zeros(B * Nq, C, device="cuda")
    ops.attention_oproj_resid_(dev(q, torch.bfloat16).view(B * Nq, C), dev(k, torch.bfloat16).view(B * Nk, C), dev(v, torch.bfloat16).view(B * Nk, C),
                               B, H, Nq, Nk, dh, dev(torch.eye(C), torch.bfloat16), torch.zeros(C, device="cuda"), x)
    kc.assert_elementwise(x, dev(want).double().reshape(B * Nq, C), 0.0, "gather probe, attention + o-proj B %d H %d Nq %d Nk %d" % (B, H, Nq, Nk))


@pytest.mark.parametrize("B,H,Nq,Nk,gated", [(3, 4, 2048, 256, False), (2, 4, 256, 2048, True), (3, 2, 8, 64, True), (2, 4, 200, 100, True),
                                              (64, 4, 256, 256, True), (128, 2, 130, 8, False)])
def test_attention_oproj_bound_vs_float64(B, H, Nq, Nk, gated):
    """randn data through the fused attention + output projection + gated residual kernel, per element: O carries its bf16 rounding and that of P
    (2^-8 (|O| + max_j |v_j|)) through |Wo|, the projection its fp32 accumulation over C terms, the update its gate."""
    dh = 32
    C = H * dh
    g = torch.Generator().manual_seed(B * 1000 + Nq + Nk + 1)
    q = dev(torch.randn(B * Nq, C, generator=g), torch.bfloat16); kv = dev(torch.randn(B * Nk, 2 * C, generator=g), torch.bfloat16)
    wo = dev(torch.randn(C, C, generator=g) / C ** 0.5, torch.bfloat16).contiguous(); bo = dev(torch.randn(C, generator=g) * 0.1)
    x0 = dev(torch.randn(B * Nq, C, generator=g))
    gate = dev(torch.randn(B, 3 * C, generator=g)) if gated else None
    att, vmax = _attention_ref64(q, kv[:, :C], kv[:, C:], B, H, Nq, Nk, dh)
    o = att.reshape(B * Nq, C)                                          # quirk Q1: [B][H][Nq][Dh] re-read raw as (B Nq, C) rows
    e_o = (kc.U8 * (att.abs() + vmax)).reshape(B * Nq, C)
    wa = wo.double().abs()
    upd = o @ wo.double().T + bo.double()
    e_u = 1.01 * (e_o @ wa.T) + C * kc.U24 * (o.abs() @ wa.T + bo.double().abs())
    gf = gate[:, C:2 * C].double().repeat_interleave(Nq, 0) if gated else None
    if gated:
        upd, e_u = gf * upd, gf.abs() * e_u
    x = x0.clone()
    ops.attention_oproj_resid_(q, kv[:, :C], kv[:, C:], B, H, Nq, Nk, dh, wo, bo, x, gate=gate[:, C:2 * C] if gated else None,
                               gate_sample_stride=3 * C if gated else 0)
    tol = e_u + 2 * kc.U24 * (x0.double().abs() + upd.abs())
    r = kc.assert_elementwise(x, x0.double() + upd, tol, "attention + o-proj B %d H %d Nq %d Nk %d" % (B, H, Nq, Nk))
    print("worst err / tol %.3f (attention + o-proj)" % note("attention + o-proj fp32 out", r))


def _attention_ref64(q, k, v, B, H, Nq, Nk, dh):
    sp = lambda z, n: z.double().reshape(B, n, H, dh).permute(0, 2, 1, 3)
    p = (sp(q, Nq) @ sp(k, Nk).transpose(-1, -2) * dh ** -0.5).softmax(-1)
    vv = sp(v, Nk)
    return (p @ vv).contiguous(), vv.abs().amax(2, keepdim=True)        # O [B, H, Nq, dh]; max_j |v_j| per (b, h, channel)


@pytest.mark.parametrize("B,H,Nq,Nk,dh,route", ATTN)
def test_attention_bound_vs_float64(B, H, Nq, Nk, dh, route):
    """randn data: |out - ref| <= 2^-8 |ref| (bf16 output) + 2^-8 max_j |v_j| (P rounded to bf16 before P V)."""
    assert _route(B, H, Nq, Nk, dh) == route
    g = torch.Generator().manual_seed(Nq * 3 + Nk)
    C = H * dh
    q = dev(torch.randn(B, Nq, C, generator=g), torch.bfloat16); kv = dev(torch.randn(B, Nk, 2 * C, generator=g) * 1.5, torch.bfloat16)
    ref, vmax = _attention_ref64(q, kv[..., :C], kv[..., C:], B, H, Nq, Nk, dh)
    out = ops.attention_fwd(q.view(B * Nq, C), kv.view(B * Nk, 2 * C)[:, :C], kv.view(B * Nk, 2 * C)[:, C:], B, H, Nq, Nk, dh)
    tol = (kc.U8 * ref.abs() + kc.U8 * vmax).reshape(-1, dh)
    r = kc.assert_elementwise(out.reshape(-1, dh), ref.reshape(-1, dh), tol, "attention route %d, B %d H %d Nq %d Nk %d Dh %d" % (route, B, H, Nq, Nk, dh))
    print("worst err / tol %.3f (attention route %d)" % (note("attention bf16 out", r), route))


# ------------------------------------------------------------------------------------------------------------- leading dimensions + guard bands
SENT_F32 = -1.7014636e38                            # bit patterns no kernel under test produces
SENT_BF16 = -1.7014118e38


def embed(t, top=8, left=64, bottom=8, right=64):
    """t as the interior of a larger NaN-surrounded tensor (offsets keep 16-byte alignment and ld % 8 == 0) -> the interior view."""
    big = torch.full((t.shape[0] + top + bottom, t.shape[1] + left + right), float("nan"), dtype=t.dtype, device=t.device)
    big[top:top + t.shape[0], left:left + t.shape[1]] = t
    return big[top:top + t.shape[0], left:left + t.shape[1]]


def guarded(shape, dtype, fill=None, top=8, left=64, bottom=8, right=64):
    """-> (big, interior view): an output buffer pre-filled with a sentinel (or `fill` in the interior)."""
    sent = SENT_BF16 if dtype == torch.bfloat16 else SENT_F32
    big = torch.full((shape[0] + top + bottom, shape[1] + left + right), sent, dtype=dtype, device="cuda")
    view = big[top:top + shape[0], left:left + shape[1]]
    if fill is not None:
        view.copy_(fill)
    return big, view


def assert_guard_intact(big, view, what, top=8, left=64):
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[top:top + view.shape[0], left:left + view.shape[1]] = False
    sent = torch.full((), SENT_BF16 if big.dtype == torch.bfloat16 else SENT_F32, dtype=big.dtype, device=big.device)
    touched = mask & (big != sent)
    if bool(touched.any()):
        idx = torch.nonzero(touched)
        raise AssertionError("%s: %d sentinel elements outside the output were overwritten, first at big[%d, %d] (interior starts at [%d, %d], is %s)"
                             % (what, idx.shape[0], int(idx[0, 0]), int(idx[0, 1]), top, left, tuple(view.shape)))
    assert not bool(torch.isnan(view.float()).any()), "%s: NaN from outside an operand reached the result" % what


@pytest.mark.parametrize("M,N,K,family", [(16384, 1024, 1024, "256-one-tile"), (16384, 3072, 1024, "256-multi-tile"), (1960, 4096, 320, "mid"),
                                         (2000, 1024, 192, "mid"), (1000, 1024, 704, "mid"), (5000, 1720, 64, "v1"), (130, 132, 64, "v1")])
def test_gemm_leading_dims_and_guard_bands(M, N, K, family):
    """ldx > K, ldw > K, ldo > N (all inside the ABI contract): operands as interiors of NaN-surrounded buffers, outputs as interiors of
    sentinel-filled ones.  The interior must equal the dense call bit for bit (same route, asserted), the sentinels must survive."""
    g = torch.Generator().manual_seed(M + N + K + 1)
    x = dev(torch.randn(M, K, generator=g), torch.bfloat16); w = dev(torch.randn(N, K, generator=g) / K ** 0.5, torch.bfloat16)
    bias = dev(torch.randn(N, generator=g)); resid = dev(torch.randn(M, N, generator=g))
    gate = dev(torch.randn(1, N, generator=g))
    xe, we = embed(x), embed(w)
    for epi in ("BF16", "GELU", "F32", "RESID"):
        dense_route = ops.gemm_route(EPI[epi], M, N, K)
        assert dense_route.family == family and ops.gemm_route(EPI[epi], M, N, K, ldo=N + 128) == dense_route
        odt = torch.bfloat16 if epi in ("BF16", "GELU") else torch.float32
        what = "%s %dx%dx%d in larger buffers" % (epi, M, N, K)
        if epi == "RESID":
            dense = resid.clone()
            ops.gemm_bf16(x, w, bias, EPI[epi], out=dense, resid=dense, gate=gate, rows_per_sample=M)
            big, view = guarded((M, N), odt, fill=resid)
            ops.gemm_bf16(xe, we, bias, EPI[epi], out=view, resid=view, gate=gate, rows_per_sample=M)
        else:
            dense = ops.gemm_bf16(x, w, bias, EPI[epi])
            big, view = guarded((M, N), odt)
            ops.gemm_bf16(xe, we, bias, EPI[epi], out=view)
        assert_guard_intact(big, view, what)
        kc.assert_elementwise(view, dense.double(), 0.0, what + " vs the dense call")


@pytest.mark.parametrize("B,H,Nq,Nk,dh,route", [(2, 4, 300, 77, 32, 0), (2, 2, 8, 5, 64, 1), (2, 2, 255, 65, 64, 2)])
def test_attention_leading_dims_and_guard_bands(B, H, Nq, Nk, dh, route):
    assert _route(B, H, Nq, Nk, dh) == route
    g = torch.Generator().manual_seed(Nq + Nk + dh)
    C = H * dh
    q = dev(torch.randn(B * Nq, C, generator=g), torch.bfloat16); k = dev(torch.randn(B * Nk, C, generator=g), torch.bfloat16)
    v = dev(torch.randn(B * Nk, C, generator=g), torch.bfloat16)
    dense = ops.attention_fwd(q, k, v, B, H, Nq, Nk, dh)
    # rows of q / k / v inside wider NaN-filled rows (no rows above / below: the batch stride is rows x ld); k and v share one buffer
    qe = embed(q, top=0, bottom=0)
    kvb = torch.full((B * Nk, 2 * C + 192), float("nan"), dtype=torch.bfloat16, device="cuda")
    kvb[:, 64:64 + C] = k; kvb[:, 128 + C:128 + 2 * C] = v
    big = torch.full((B * H * Nq * dh + 512,), SENT_BF16, dtype=torch.bfloat16, device="cuda")
    out = big[256:256 + B * H * Nq * dh].view(B, H, Nq, dh)
    ops.attention_fwd(qe, kvb[:, 64:64 + C], kvb[:, 128 + C:128 + 2 * C], B, H, Nq, Nk, dh, out=out)
    what = "attention route %d in larger buffers" % route
    sent = torch.full((), SENT_BF16, dtype=torch.bfloat16, device="cuda")
    assert bool((big[:256] == sent).all()) and bool((big[256 + B * H * Nq * dh:] == sent).all()), what + ": wrote outside O"
    assert not bool(torch.isnan(out.float()).any()), what + ": NaN from outside an operand reached the result"
    kc.assert_elementwise(out.reshape(-1, dh), dense.double().reshape(-1, dh), 0.0, what + " vs the dense call")


@pytest.mark.parametrize("M,C", [(64, 1024), (33, 64), (5, 96)])
def test_layernorm_modulate_and_cast_pad_guard_bands(M, C):
    g = torch.Generator().manual_seed(M + C)
    x = dev(torch.randn(M, C, generator=g) * 3 + 1)
    mod = dev(torch.randn(M, 2 * C, generator=g) * 0.5)
    kw = dict(shift=mod[:, :C], scale=mod[:, C:], mod_sample_stride=2 * C, rows_per_sample=1)
    dense = ops.layernorm_modulate(x, **kw)
    big, view = guarded((M, C), torch.bfloat16)
    ops.layernorm_modulate(embed(x), out=view, **kw)
    assert_guard_intact(big, view, "layernorm_modulate %dx%d in larger buffers" % (M, C))
    kc.assert_elementwise(view, dense.double(), 0.0, "layernorm_modulate %dx%d in larger buffers vs the dense call" % (M, C))
    # against float64: LayerNorm in fp32 (2^-20 on a normalised value of a few units) + modulation + the bf16 output
    xd = x.double()
    h = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-6)
    ref = h * (1 + mod[:, C:].double()) + mod[:, :C].double()
    tol = 2.0 ** -20 * (1 + h.abs()) * (1 + mod[:, C:].double().abs()) * 4 + kc.U8 * ref.abs() * (1 + kc.U8)
    note("layernorm_modulate bf16 out", kc.assert_elementwise(dense, ref, tol, "layernorm_modulate %dx%d" % (M, C)))
    # cast_pad_bf16: cols -> cols_pad zero padded; exact (round to nearest even)
    pad = ops.pad64(C + 3)
    src = dev(torch.randn(M, C + 3, generator=g))
    dense = ops.cast_pad_bf16(src, pad)
    big, view = guarded((M, pad), torch.bfloat16)
    ops.cast_pad_bf16(embed(src), pad, out=view)
    assert_guard_intact(big, view, "cast_pad_bf16 %dx%d" % (M, C + 3))
    assert torch.equal(view, dense) and torch.equal(dense[:, :C + 3], src.bfloat16()) and not bool(dense[:, C + 3:].any())


@pytest.mark.parametrize("C,M,N", [(128, 333, 384), (64, 1000, 64)])
def test_ln_linear_and_ln_mlp_guard_bands_and_bounds(C, M, N):
    """The narrow fused kernels: x as the interior of a NaN-surrounded buffer (ldx > C) == the dense call bit for bit, the in-place update and
    the bf16 mirror leave their surround alone; and against float64 per element (the hidden layer's bf16 rounding propagated through |W2|)."""
    g = torch.Generator().manual_seed(C + M + N)
    x = dev(torch.randn(M, C, generator=g) * 1.5 - 0.2)
    lw, lb = dev(torch.rand(C, generator=g) + 0.5), dev(torch.randn(C, generator=g) * 0.2)
    w = dev(torch.randn(N, C, generator=g) / C ** 0.5, torch.bfloat16).contiguous(); b = dev(torch.randn(N, generator=g) * 0.1)
    dense = ops.ln_linear(x, w, b, ln_w=lw, ln_b=lb)
    got = ops.ln_linear(embed(x), w, b, ln_w=lw, ln_b=lb)
    assert not bool(torch.isnan(got.float()).any())
    kc.assert_elementwise(got, dense.double(), 0.0, "ln_linear C %d M %d N %d with ldx > C vs the dense call" % (C, M, N))
    xd = x.double()
    h = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-6) * lw.double() + lb.double()
    ref = h @ w.double().T + b.double()
    # h is rounded to bf16 before the MFMA: 2^-8 |h| through |W|; fp32 accumulation over C terms; the bf16 output
    tol = (kc.U8 * 1.01) * (h.abs() @ w.double().abs().T) + C * kc.U24 * (h.abs() @ w.double().abs().T + b.double().abs()) + kc.U8 * ref.abs()
    note("ln_linear bf16 out", kc.assert_elementwise(dense, ref, tol, "ln_linear C %d M %d N %d" % (C, M, N)))
    # beside that bound (its 2^-8 |h| |W| is as large as an output ulp): the interval of the staged reference, which pins most elements to the bit
    kc.check_ln_linear(dense, kc.ln_linear_reference(x, w.float(), b, ln_w=lw, ln_b=lb), "ln_linear C %d M %d N %d, staged" % (C, M, N))
    # ---- ln_mlp_resid_
    w_up = dev(torch.randn(4 * C, C, generator=g) / C ** 0.5, torch.bfloat16).contiguous(); b_up = dev(torch.randn(4 * C, generator=g) * 0.1)
    w_dn = dev(torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5, torch.bfloat16).contiguous(); b_dn = dev(torch.randn(C, generator=g) * 0.1)
    x1 = x.clone()
    ops.ln_mlp_resid_(x1, w_up, b_up, w_dn, b_dn, ln_w=lw, ln_b=lb)
    big, view = guarded((M, C), torch.float32, fill=x)
    mbig, mirror = guarded((M, C), torch.bfloat16)
    ops.ln_mlp_resid_(view, w_up, b_up, w_dn, b_dn, ln_w=lw, ln_b=lb, x_bf16_out=mirror)
    assert_guard_intact(big, view, "ln_mlp_resid_ C %d M %d in place inside a larger buffer" % (C, M))
    assert_guard_intact(mbig, mirror, "ln_mlp_resid_ C %d M %d bf16 mirror" % (C, M))
    kc.assert_elementwise(view, x1.double(), 0.0, "ln_mlp_resid_ C %d M %d with ldx > C vs the dense call" % (C, M))
    assert torch.equal(mirror, x1.bfloat16())
    a1 = h.abs() @ w_up.double().abs().T
    u = h @ w_up.double().T + b_up.double()
    e_u = (kc.U8 * 1.01) * a1 + C * kc.U24 * (a1 + b_up.double().abs())                      # error of the hidden pre-activation
    gu = torch.nn.functional.gelu(u)
    e_g = e_u * kc.GELU_SLOPE + kc.GELU_FAST_ABS + kc.U8 * 1.01 * gu.abs()                   # ... of the bf16 hidden activation
    upd = gu @ w_dn.double().T + b_dn.double()
    a2 = gu.abs() @ w_dn.double().abs().T
    tol = e_g @ w_dn.double().abs().T + 4 * C * kc.U24 * (a2 + b_dn.double().abs()) + 2 * kc.U24 * (xd.abs() + upd.abs())
    note("ln_mlp_resid_ fp32 out", kc.assert_elementwise(x1, xd + upd, tol, "ln_mlp_resid_ C %d M %d" % (C, M)))
    # beside that bound (2^-8 per bf16 stage: as large as the update itself): the staged reference, hundreds of times tighter
    sr = kc.fused_mlp_reference(x, w_up.float(), b_up, w_dn.float(), b_dn, ln_w=lw, ln_b=lb)
    note("ln_mlp_resid_ fp32 out, staged", kc.check_fused_mlp(x1, sr, "ln_mlp_resid_ C %d M %d, staged" % (C, M)))
    assert float((tol / sr["tol"]).median()) > 50


def test_zz_margins():
    """Not a check: prints the worst err / tol of every class of bound above (the numbers DESIGN.md quotes)."""
    for k in sorted(RATIOS):
        print("worst err / tol, %-40s %.3f   (C_ACC = %g)" % (k + ":", RATIOS[k], kc.C_ACC))
