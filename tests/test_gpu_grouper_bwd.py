"""GPU (-m gpu): the backward of the grouper's data movement alone (ldt_maxpool_argmax, ldt_maxpool_relu_bwd, ldt_group_normalize_bwd:
csrc/grouper_bwd.hip).  The cases, the float64 references and the bounds: tests/front_train_checks.py.

  * the max with its arg-max: the values are ldt_maxpool's bit for bit; planted ties (the smallest index wins), positive ones and cells whose
    every row is 0; bf16 and fp32 inputs; its backward routes d_out to the kept row where out > 0 and writes 0 everywhere else: torch.equal
  * ldt_group_normalize_bwd at (B, n, S, k, D) = (1, 5, 1, 2, 3), (3, 64, 8, 16, 64) the tiny fixture, (2, 300, 7, 12, 128) ragged at the
    shipped width, (2, 2048, 32, 128, 128) the shipped per-sample shape: dalpha, dbeta and dfeat per element against float64; one point sits
    in every group, one point in no group (its gradient exactly 0), every centre among its own neighbours; fp32 and bf16 dU
  * guard bytes around every output; a second call repeats bit for bit
  * the refusals

Before the kernels existed every test here ended at the missing `ops.maxpool_argmax` / `ops.group_normalize_bwd`."""
import pytest
import torch

import front_train_checks as fc
import kernel_checks as kc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("G,n,C,bf16", [(1, 1, 5, False), (24, 16, 64, True), (3, 8, 256, False), (14, 12, 131, True), (64, 128, 128, True)])
def test_maxpool_argmax_and_its_backward(G, n, C, bf16):
    from ldt_amd import ops
    x = fc.maxpool_case(G, n, C, seed=100 + G + C, bf16=bf16)
    xd = x.bfloat16().cuda() if bf16 else x.cuda()
    out, arg = ops.maxpool_argmax(xd, G, n)
    want, want_arg = fc.maxpool_argmax_ref(x, G, n)
    assert torch.equal(out, ops.maxpool(xd, G, n)) and torch.equal(out.cpu(), want)
    assert torch.equal(arg.cpu(), want_arg)
    if n > 1:
        assert not torch.equal(want_arg, fc.maxpool_argmax_ref(x, G, n, last_wins=True)[1])          # the ties are there
        assert bool((want == 0).any()) and bool((want > 0).any())
    out2, arg2 = ops.maxpool_argmax(xd, G, n)
    assert torch.equal(out2, out) and torch.equal(arg2, arg)
    # relu: ReLU(max_j z_j) = max_j ReLU(z_j) with the arg-max of z itself, on rows that are NOT ReLU outputs (cells whose maximum is negative)
    zs = x - 0.75
    zs = zs.bfloat16().float() if bf16 else zs
    zd = zs.bfloat16().cuda() if bf16 else zs.cuda()
    out_r, arg_r = ops.maxpool_argmax(zd, G, n, relu=True)
    want_r, want_arg_r = fc.maxpool_argmax_ref(zs, G, n)
    assert torch.equal(out_r.cpu(), want_r.clamp_min(0)) and torch.equal(arg_r.cpu(), want_arg_r) and torch.equal(ops.maxpool_argmax(zd, G, n)[0].cpu(), want_r)
    assert n == 1 or (bool((want_r < 0).any()) and bool((out_r > 0).any()))
    g = torch.Generator().manual_seed(5)
    d_out = torch.randn(G, C, generator=g)
    big, dz = kc.guarded(G * n, C, 7.0, "cuda")
    assert ops.maxpool_relu_bwd(d_out.cuda(), out, arg, n, dz=dz) is dz
    ref = fc.maxpool_relu_bwd_ref(d_out, want, want_arg, n)
    assert torch.equal(dz.cpu(), ref)
    kc.assert_guard_intact(big, G * n * C, "maxpool_relu_bwd (%d, %d, %d)" % (G, n, C))
    # against autograd of max(relu(z)): the same routing wherever the maximum is positive and unique
    z = x.clone().view(G, n, C).requires_grad_(True)
    torch.relu(z).max(1).values.backward(d_out)
    uniq = ((x.view(G, n, C) == want[:, None, :]).sum(1) == 1) & (want > 0)
    assert torch.equal(torch.where(uniq[:, None, :], ref.view(G, n, C), torch.zeros(())), torch.where(uniq[:, None, :], z.grad, torch.zeros(())))


def run_gnb(c, dU):
    from ldt_amd import ops
    B, n, D = c["B"], c["n"], c["D"]
    out = ops.group_normalize_bwd(dU, c["feat"].cuda(), c["xyz"].cuda(), c["fi"].cuda(), c["ki"].cuda(), c["alpha"].cuda())
    assert tuple(out[0].shape) == (D + 3,) and tuple(out[1].shape) == (D + 3,) and tuple(out[2].shape) == (B, n, D)
    return out


@pytest.mark.parametrize("B,n,S,k,D", fc.GNB_CASES)
@pytest.mark.parametrize("bf16", [False, True])
def test_group_normalize_bwd_per_element(B, n, S, k, D, bf16):
    from ldt_amd import ops
    c = fc.gnb_case(B, n, S, k, D, bf16=bf16)
    what = "group_normalize_bwd (%d, %d, %d, %d, %d)%s" % (B, n, S, k, D, " bf16 dU" if bf16 else "")
    ki = c["ki"].long()
    assert bool((ki == c["all"]).any(2).all()) and not bool((ki == c["none"]).any()) and not bool((c["fi"] == c["none"]).any())
    assert bool((ki == c["fi"].long()[:, :, None]).any(2).all())
    ref, tol = fc.group_normalize_bwd_ref(c)
    got = run_gnb(c, c["dU"].cuda())
    r = [kc.assert_elementwise(g.cpu(), w, t, "%s %s" % (what, nm)) for g, w, t, nm in zip(got, ref, tol, ("dalpha", "dbeta", "dfeat"))]
    print("train-kernel %s  max err/tol  dalpha %.3f  dbeta %.3f  dfeat %.3f" % ((what,) + tuple(r)))
    assert bool((got[2][:, c["none"]] == 0).all()) and float(ref[2][:, c["all"]].abs().min()) > 0
    again = run_gnb(c, c["dU"].cuda())
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    # a wider row stride (the padded grouped rows) and dfeat skipped: the same bits
    wide = torch.zeros(c["dU"].shape[0], kc.pad64(2 * D + 3) + 64, dtype=c["dU"].dtype, device="cuda")
    wide[:, :2 * D + 3] = c["dU"].cuda()
    w = run_gnb(c, wide)
    assert all(torch.equal(a, b) for a, b in zip(w, got))
    only = ops.group_normalize_bwd(wide, c["feat"].cuda(), c["xyz"].cuda(), c["fi"].cuda(), c["ki"].cuda(), c["alpha"].cuda(), want_dfeat=False)
    assert only[2] is None and torch.equal(only[0], got[0]) and torch.equal(only[1], got[1])


def test_group_normalize_bwd_guards_and_the_inverted_index():
    from ldt_amd import ops
    from ldt_amd._lib import lib
    B, n, S, k, D = 3, 64, 8, 16, 64
    c = fc.gnb_case(B, n, S, k, D)
    start, entry = ops.knn_inverted_index(c["ki"].cuda(), n)
    flat = c["ki"].view(B, -1).long()
    for b in range(B):
        for p in (0, c["all"], c["none"], 17):
            want = torch.nonzero(flat[b] == p).flatten().int()
            assert torch.equal(entry[b, int(start[b, p]):int(start[b, p + 1])].cpu(), want)
    assert bool((start[:, 0] == 0).all()) and bool((start[:, n] == S * k).all())
    ba, da = kc.guarded(1, D + 3, 0.0, "cuda")
    bb, db = kc.guarded(1, D + 3, 0.0, "cuda")
    bf, df = kc.guarded(B * n, D, 0.0, "cuda")
    t = lambda x: x.cuda().contiguous()
    dU, feat, xyz, fi, ki, al = t(c["dU"]), t(c["feat"]), t(c["xyz"]), t(c["fi"]), t(c["ki"]), t(c["alpha"])
    p, s = (lambda x: x.data_ptr()), torch.cuda.current_stream().cuda_stream
    f = lib().ldt_group_normalize_bwd
    assert f(p(dU), 0, dU.stride(0), p(feat), p(xyz), p(fi), p(ki), p(start), p(entry), p(al), B, n, S, k, D, p(da), p(db), p(df), s) == 0
    got = ops.group_normalize_bwd(dU, feat, xyz, fi, ki, al, index=(start, entry))
    assert torch.equal(da.view(-1), got[0]) and torch.equal(db.view(-1), got[1]) and torch.equal(df.view(B, n, D), got[2])
    for big, numel, nm in ((ba, D + 3, "dalpha"), (bb, D + 3, "dbeta"), (bf, B * n * D, "dfeat")):
        kc.assert_guard_intact(big, numel, "group_normalize_bwd " + nm)
    # refusals: status codes before any launch
    assert f(None, 0, dU.stride(0), p(feat), p(xyz), p(fi), p(ki), p(start), p(entry), p(al), B, n, S, k, D, p(da), p(db), p(df), s) == -1
    assert f(p(dU), 0, dU.stride(0), p(feat), p(xyz), p(fi), p(ki), None, p(entry), p(al), B, n, S, k, D, p(da), p(db), p(df), s) == -1
    assert f(p(dU), 0, 2 * D + 2, p(feat), p(xyz), p(fi), p(ki), p(start), p(entry), p(al), B, n, S, k, D, p(da), p(db), p(df), s) == -2
    assert f(p(dU), 0, dU.stride(0), p(feat), p(xyz), p(fi), p(ki), p(start), p(entry), p(al), B, n, 0, k, D, p(da), p(db), p(df), s) == -2
    L = lib()
    o, a = torch.zeros(2, 8, device="cuda"), torch.zeros(2, 8, dtype=torch.int32, device="cuda")
    assert L.ldt_maxpool_argmax(None, 0, 8, 2, 4, 8, p(o), p(a), 0, s) == -1 and L.ldt_maxpool_argmax(p(o), 0, 4, 2, 1, 8, p(o), p(a), 0, s) == -2
    assert L.ldt_maxpool_relu_bwd(p(o), p(o), None, 2, 1, 8, p(o), 8, s) == -1 and L.ldt_maxpool_relu_bwd(p(o), p(o), p(a), 2, 1, 8, p(o), 4, s) == -2
    with pytest.raises(ValueError, match="is not"):
        ops.group_normalize_bwd(dU[:-1], feat, xyz, fi, ki, al)
    with pytest.raises(ValueError, match="is not"):
        ops.maxpool_argmax(o, 3, 4)
    torch.cuda.synchronize()
