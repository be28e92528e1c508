"""GPU (-m gpu): training-mode BatchNorm + ReLU alone, per element against float64 (ldt_bn_stats, ldt_bn_relu_fwd, ldt_bn_relu_bwd:
csrc/batchnorm.hip).  The cases, the float64 references and the bounds counted from the kernels' operation order:
tests/front_train_checks.py.

  * (M, C) = (2, 5) the smallest M and an odd width, (384, 64) the tiny fixture's M, (4101, 131) a row tail and a width that is no multiple
    of 4 (the scalar form), (512, 256) MiniPointnet, (70 000, 128) past the shipped 65 536 rows (137 partials across workgroups)
  * a column of variance 0: rstd = 1 / sqrt(eps) to the bit of its float64 value rounded once; one row's dy 2^20 times the others'
  * the running buffers as nn.BatchNorm1d updates them (momentum 0.1, unbiased variance), against torch's own module too
  * the backward's mask is the forward's: (y > 0) of ldt_bn_relu_fwd's fp32 output == the restated fp32 arithmetic, cell for cell
  * guard bytes around every output; a second call repeats bit for bit; dx aliasing dy: the same bits; a misaligned x takes the scalar
    form of the same kernels: the same bits
  * the refusals: M = 1, null pointers, the wrapper's shape errors

Before the kernels existed every test here ended at the missing `ops.bn_stats`."""
import pytest
import torch

import front_train_checks as fc
import kernel_checks as kc

pytestmark = pytest.mark.gpu


def run_stats(c, M, C):
    from ldt_amd import ops
    big, st = kc.guarded(2, C, 0.0, "cuda")
    bm, rm = kc.guarded(1, C, 0.0, "cuda")
    bv, rv = kc.guarded(1, C, 0.0, "cuda")
    rm.copy_(c["running_mean"].view(1, C)); rv.copy_(c["running_var"].view(1, C))
    out = ops.bn_stats(c["x"].cuda(), fc.BN_EPS, rm.view(-1), rv.view(-1), fc.BN_MOMENTUM, out=st)
    assert out is st
    for b, n, nm in ((big, 2 * C, "stats"), (bm, C, "running_mean"), (bv, C, "running_var")):
        kc.assert_guard_intact(b, n, "bn_stats (%d, %d) %s" % (M, C, nm))
    return st, rm.view(-1), rv.view(-1)


def check_stats(c, M, C, what):
    ref, tol = fc.bn_stats_ref(c["x"], c["running_mean"], c["running_var"])
    st, rm, rv = run_stats(c, M, C)
    got = {"mean": st[0], "rstd": st[1], "running_mean": rm, "running_var": rv}
    r = {k: kc.assert_elementwise(got[k].cpu(), ref[k], tol[k], "%s %s" % (what, k)) for k in ref}
    print("train-kernel %s  max err/tol  %s" % (what, "  ".join("%s %.3f" % kv for kv in r.items())))
    st2, rm2, rv2 = run_stats(c, M, C)
    assert torch.equal(st2, st) and torch.equal(rm2, rm) and torch.equal(rv2, rv)
    return st


def check_fwd_bwd(c, M, C, st, what):
    from ldt_amd import ops
    x, dy, ga, be = (c[k].cuda() for k in ("x", "dy", "gamma", "beta"))
    st_h = st.cpu()
    ratios = {}
    # forward, fp32 and bf16 (with K padding)
    ref, tol = fc.bn_relu_fwd_ref(c["x"], st_h, c["gamma"], c["beta"], False)
    big, y = kc.guarded(M, C, 0.0, "cuda")
    assert ops.bn_relu_fwd(x, st, ga, be, out=y) is y
    ratios["y"] = kc.assert_elementwise(y.cpu(), ref, tol, what + " y fp32")
    kc.assert_guard_intact(big, M * C, what + " y")
    xh, pre = fc.bn_pre_fp32(c["x"], st_h, c["gamma"], c["beta"])
    assert torch.equal(y.cpu() > 0, pre > 0), what + ": the forward's mask is not the restated fp32 arithmetic's"
    refb, tolb = fc.bn_relu_fwd_ref(c["x"], st_h, c["gamma"], c["beta"], True)
    yb = ops.bn_relu_fwd(x, st, ga, be)
    assert yb.dtype == torch.bfloat16 and tuple(yb.shape) == (M, kc.pad64(C)) and bool((yb[:, C:].float() == 0).all())
    ratios["y bf16"] = kc.assert_elementwise(yb[:, :C].float().cpu(), refb, tolb, what + " y bf16")
    assert torch.equal(ops.bn_relu_fwd(x, st, ga, be), yb)
    # backward
    ref, tol = fc.bn_relu_bwd_ref(c["dy"], c["x"], st_h, c["gamma"], c["beta"], mask=pre > 0)
    bx, dx = kc.guarded(M, C, 0.0, "cuda")
    bg, dg = kc.guarded(1, C, 0.0, "cuda")
    bb, db = kc.guarded(1, C, 0.0, "cuda")
    out = ops.bn_relu_bwd(dy, x, st, ga, be, dx=dx, dgamma=dg.view(-1), dbeta=db.view(-1))
    assert out[0] is dx
    for g, r, t, nm in zip((dx, dg.view(-1), db.view(-1)), ref, tol, ("dx", "dgamma", "dbeta")):
        ratios[nm] = kc.assert_elementwise(g.cpu(), r, t, "%s %s" % (what, nm))
    for b, n, nm in ((bx, M * C, "dx"), (bg, C, "dgamma"), (bb, C, "dbeta")):
        kc.assert_guard_intact(b, n, "%s %s" % (what, nm))
    print("train-kernel %s  max err/tol  %s" % (what, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    again = ops.bn_relu_bwd(dy, x, st, ga, be)
    assert torch.equal(again[0], dx) and torch.equal(again[1], dg.view(-1)) and torch.equal(again[2], db.view(-1))
    alias = dy.clone()
    out = ops.bn_relu_bwd(alias, x, st, ga, be, dx=alias)
    assert out[0] is alias and torch.equal(alias, dx) and torch.equal(out[1], dg.view(-1))
    return dx, dg.view(-1), db.view(-1), y


@pytest.mark.parametrize("M,C", fc.BN_CASES)
def test_bn_train_per_element(M, C):
    from ldt_amd import ops
    c = fc.bn_case(M, C)
    what = "bn (%d, %d)" % (M, C)
    st = check_stats(c, M, C, what)
    dx, dg, db, y = check_fwd_bwd(c, M, C, st, what)
    if M <= 4101:
        # a misaligned x: the scalar form of the same kernels, the same bits
        off = torch.empty(M * C + 1, device="cuda")[1:]
        off.copy_(c["x"].cuda().view(-1))
        assert off.data_ptr() % 16 == 4
        xm = off.view(M, C)
        assert torch.equal(ops.bn_stats(xm), st)
        ga, be = c["gamma"].cuda(), c["beta"].cuda()
        assert torch.equal(ops.bn_relu_fwd(xm, st, ga, be, out_bf16=False), y)
        mis = ops.bn_relu_bwd(c["dy"].cuda(), xm, st, ga, be)
        assert torch.equal(mis[0], dx) and torch.equal(mis[1], dg) and torch.equal(mis[2], db)


def test_bn_train_zero_variance_column_and_a_dominant_row():
    M, C = 700, 64
    c = fc.bn_case(M, C, seed=11, zero_var_col=5)
    st = check_stats(c, M, C, "bn (700, 64) column 5 constant")
    want = torch.tensor(fc.BN_EPS ** -0.5, dtype=torch.float64).float()
    assert float(st[1, 5]) == float(want) and float(st[0, 5]) == float(c["x"][0, 5])               # variance exactly 0
    check_fwd_bwd(c, M, C, st, "bn (700, 64) column 5 constant")
    c = fc.bn_case(M, C, seed=12, big_row=M // 2)
    st = check_stats(c, M, C, "bn (700, 64) one row 2^20")
    check_fwd_bwd(c, M, C, st, "bn (700, 64) one row 2^20")


def test_bn_stats_against_torch_batchnorm1d():
    """The module itself in training mode on the CPU: batch statistics through its output, the buffers after one step."""
    M, C = 384, 64
    c = fc.bn_case(M, C, seed=3)
    bn = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        bn.weight.copy_(c["gamma"]); bn.bias.copy_(c["beta"]); bn.running_mean.copy_(c["running_mean"]); bn.running_var.copy_(c["running_var"])
    bn.train()
    y = torch.relu(bn(c["x"])).detach()
    st, rm, rv = run_stats(c, M, C)
    from ldt_amd import ops
    got = ops.bn_relu_fwd(c["x"].cuda(), st, c["gamma"].cuda(), c["beta"].cuda(), out_bf16=False)
    assert float((got.cpu() - y).abs().max()) <= 1e-5 * float(y.abs().max())
    assert float((rm.cpu() - bn.running_mean).abs().max()) <= 1e-6 and float((rv.cpu() - bn.running_var).abs().max()) <= 1e-5


def test_bn_refusals():
    from ldt_amd import ops
    from ldt_amd._lib import lib
    x = torch.zeros(4, 8, device="cuda")
    st, v = torch.zeros(2, 8, device="cuda"), torch.ones(8, device="cuda")
    p, s = (lambda t: t.data_ptr()), torch.cuda.current_stream().cuda_stream
    L = lib()
    assert L.ldt_bn_stats(None, 8, 4, 8, 1e-5, p(st), None, None, 0.1, s) == -1
    assert L.ldt_bn_stats(p(x), 8, 1, 8, 1e-5, p(st), None, None, 0.1, s) == -2                     # one value per channel
    assert L.ldt_bn_stats(p(x), 4, 4, 8, 1e-5, p(st), None, None, 0.1, s) == -2
    assert L.ldt_bn_stats(p(x), 8, 4, 8, 1e-5, p(st), None, None, 1.5, s) == -1
    assert L.ldt_bn_relu_fwd(p(x), 8, 4, 8, p(st), p(v), None, p(x), 8, 0, 8, s) == -1
    assert L.ldt_bn_relu_fwd(p(x), 8, 4, 8, p(st), p(v), p(v), p(x), 8, 0, 4, s) == -2
    assert L.ldt_bn_relu_bwd(p(x), 8, p(x), 8, 1, 8, p(st), p(v), p(v), p(x), 8, None, None, s) == -2
    assert L.ldt_bn_relu_bwd(p(x), 8, None, 8, 4, 8, p(st), p(v), p(v), p(x), 8, None, None, s) == -1
    with pytest.raises(ValueError, match="more than one value per channel"):
        ops.bn_stats(x[:1])
    with pytest.raises(ValueError, match="stats must be"):
        ops.bn_relu_fwd(x, st[:, :4].contiguous(), v, v)
    with pytest.raises(ValueError, match="gamma"):
        ops.bn_relu_fwd(x, st, v[:4], v)
    with pytest.raises(ValueError, match="share one"):
        ops.bn_relu_bwd(x[:, :4].contiguous(), x, st, v, v)
    with pytest.raises(TypeError):
        ops.bn_stats(x.double())
    torch.cuda.synchronize()
