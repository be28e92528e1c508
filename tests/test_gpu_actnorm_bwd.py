"""GPU (-m gpu): the ActNorm backward alone, per element against float64 (ldt_actnorm_bwd: csrc/actnorm.hip).  The cases, the float64
reference and the bounds counted from the kernel's operation order: tests/encoder_train_checks.py (dx: two roundings plus the libm
constant of expf; the sums: one final rounding plus the summed bounds of their terms).

  * (B, per_sample) = (1, 5), (3, 8 x 64), (16, 32 x 128) the shipped per-token form, (2, 4101) the scalar form with its tail, (700, 64)
    and (5000, 64) the 'set' form past one workgroup's 512 rows (the second stage adds 2 and 10 partials)
  * guard bytes around dx, dshift and dlog_scale; a second call repeats bit for bit
  * a misaligned dz takes the scalar form of the same kernel: the same bits; dx aliasing dz: the same bits; the sums skipped: the same dx
  * log_scale up to +-3; one sample's dz 2^20 times the others'
  * the refusals: LDT_EARG from the entry point, the wrapper's shape errors

Before ldt_actnorm_bwd existed every test here ended at the missing `ops.actnorm_bwd`."""
import pytest
import torch

import encoder_train_checks as ec
import kernel_checks as kc

pytestmark = pytest.mark.gpu


def run(c, B, per, **kw):
    """-> ((dx, dshift, dlog_scale) on the device, the three guarded surrounds)."""
    from ldt_amd import ops
    bx, dx = kc.guarded(B, per, 0.0, "cuda")
    bs, ds = kc.guarded(1, per, 0.0, "cuda")
    bl, dl = kc.guarded(1, per, 0.0, "cuda")
    out = ops.actnorm_bwd(c["dz"].cuda(), c["z"].cuda(), c["log_scale"].cuda(), B, dx=dx, dshift=ds.view(-1), dlog_scale=dl.view(-1), **kw)
    assert out[0] is dx
    return (dx, ds.view(-1), dl.view(-1)), (bx, bs, bl)


def check_guards(bigs, B, per, what):
    for big, n, nm in zip(bigs, (B * per, per, per), ("dx", "dshift", "dlog_scale")):
        kc.assert_guard_intact(big, n, "%s %s" % (what, nm))


@pytest.mark.parametrize("B,per", ec.ANB_CASES)
def test_actnorm_bwd_per_element(B, per):
    from ldt_amd import ops
    c = ec.actnorm_case(B, per)
    ref, tol = ec.actnorm_bwd_ref(c["dz"], c["z"], c["log_scale"])
    what = "actnorm_bwd (%d, %d)" % (B, per)
    got, bigs = run(c, B, per)
    r = ec.actnorm_worst([t.cpu().view_as(w) for t, w in zip(got, ref)], ref, tol, what)
    print("train-kernel %s  max err/tol  dx %.3f  dshift %.3f  dlog_scale %.3f" % ((what,) + r))
    check_guards(bigs, B, per, what)
    again, _ = run(c, B, per)
    assert all(torch.equal(a, b) for a, b in zip(again, got))                                   # fixed order everywhere: the same bits
    dz_d, z_d, ls_d = c["dz"].cuda(), c["z"].cuda(), c["log_scale"].cuda()
    # fresh buffers
    fresh = ops.actnorm_bwd(dz_d, z_d, ls_d, B)
    assert tuple(fresh[0].shape) == (B, per) and tuple(fresh[1].shape) == (per,) and all(torch.equal(a.view(-1), b.view(-1)) for a, b in zip(fresh, got))
    # a misaligned dz: the scalar form of the same kernel, the same bits
    off = torch.empty(B * per + 1, device="cuda")[1:]
    off.copy_(dz_d.view(-1))
    assert off.data_ptr() % 16 == 4
    mis = ops.actnorm_bwd(off.view(B, per), z_d, ls_d, B)
    assert all(torch.equal(a.view(-1), b.view(-1)) for a, b in zip(mis, got))
    # dx aliasing dz
    alias = dz_d.clone()
    out = ops.actnorm_bwd(alias, z_d, ls_d, B, dx=alias)
    assert out[0] is alias and all(torch.equal(a.view(-1), b.view(-1)) for a, b in zip(out, got))
    # the sums skipped: dx only
    bx, dx = kc.guarded(B, per, 0.0, "cuda")
    only = ops.actnorm_bwd(dz_d, z_d, ls_d, B, dx=dx, want_sums=False)
    assert only[1] is None and only[2] is None and torch.equal(dx, got[0])
    kc.assert_guard_intact(bx, B * per, what + " dx alone")


@pytest.mark.parametrize("B,per", [(3, 8 * 64), (700, 64), (2, 4101)])
def test_actnorm_bwd_wide_log_scale_and_a_dominant_sample(B, per):
    what = "actnorm_bwd (%d, %d)" % (B, per)
    c = ec.actnorm_case(B, per, ls_max=3.0, seed=7)
    assert float(c["log_scale"].max()) == 3.0 and float(c["log_scale"].min()) == -3.0
    ref, tol = ec.actnorm_bwd_ref(c["dz"], c["z"], c["log_scale"])
    got, bigs = run(c, B, per)
    r = ec.actnorm_worst([t.cpu().view_as(w) for t, w in zip(got, ref)], ref, tol, what + " log_scale +-3")
    print("train-kernel %s log_scale +-3  max err/tol  dx %.3f  dshift %.3f  dlog_scale %.3f" % ((what,) + r))
    check_guards(bigs, B, per, what)
    c = ec.actnorm_case(B, per, seed=8, big_sample=B // 2)
    ref, tol = ec.actnorm_bwd_ref(c["dz"], c["z"], c["log_scale"])
    got, bigs = run(c, B, per)
    r = ec.actnorm_worst([t.cpu().view_as(w) for t, w in zip(got, ref)], ref, tol, what + " one sample 2^20")
    print("train-kernel %s one sample 2^20  max err/tol  dx %.3f  dshift %.3f  dlog_scale %.3f" % ((what,) + r))
    check_guards(bigs, B, per, what)


def test_actnorm_bwd_is_the_gradient_of_actnorm():
    """z from ldt_actnorm itself (in place on a copy), as the step keeps it."""
    from ldt_amd import ops
    B, per = 3, 8 * 64
    c = ec.actnorm_case(B, per)
    z = c["x"].cuda().clone()
    ops.actnorm_(z, c["shift"].cuda(), c["log_scale"].cuda(), B)
    ref, tol = ec.actnorm_bwd_ref(c["dz"], z.cpu(), c["log_scale"])
    got = ops.actnorm_bwd(c["dz"].cuda(), z, c["log_scale"].cuda(), B)
    ec.actnorm_worst([t.cpu().view_as(w) for t, w in zip(got, ref)], ref, tol, "on ldt_actnorm's own output")


def test_actnorm_bwd_refusals():
    from ldt_amd import ops
    from ldt_amd._lib import lib
    dz, z, ls = torch.zeros(2, 8, device="cuda"), torch.zeros(2, 8, device="cuda"), torch.zeros(8, device="cuda")
    f, p = lib().ldt_actnorm_bwd, lambda t: t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    assert f(None, p(z), p(ls), 2, 8, p(dz), None, None, s) == -1
    assert f(p(dz), None, p(ls), 2, 8, p(dz), None, p(ls), s) == -1
    assert f(p(dz), p(z), p(ls), 0, 8, p(dz), None, None, s) == -1 and f(p(dz), p(z), p(ls), 2, 0, p(dz), None, None, s) == -1
    with pytest.raises(ValueError, match="one shape"):
        ops.actnorm_bwd(dz, z[:, :4].contiguous(), ls, 2)
    with pytest.raises(ValueError, match="in B = 3 samples"):
        ops.actnorm_bwd(dz, z, ls, 3)
    with pytest.raises(ValueError, match="log_scale"):
        ops.actnorm_bwd(dz, z, ls[:4].contiguous(), 2)
    with pytest.raises(ValueError, match="a sum buffer"):
        ops.actnorm_bwd(dz, z, ls, 2, dshift=torch.zeros(4, device="cuda"))
    with pytest.raises(TypeError):
        ops.actnorm_bwd(dz.double(), z, ls, 2)
    torch.cuda.synchronize()
