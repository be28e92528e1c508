"""GPU (-m gpu): the Chamfer reconstruction loss alone (csrc/chamfer_loss.hip: ldt_chamfer_nn, ldt_cd_loss, ldt_cd_loss_bwd, and
ldt_amd.losses.cd_loss over them).  References and bounds: tests/decoder_train_checks.py (test_decoder_train_host.py holds them against
torch.autograd without a GPU, planted faults included).

  * distances bit-equal to ops.chamfer; every index a valid argmin (no element left out)
  * the loss, l1 and l2, within 2 x 2^-24 relative of float64 over the same distances
  * dx1 per element against the float64 gradient teacher-forced on the kernel's own indices
  * exact probes: a duplicated target yields the lower index; a coincident pair yields a gradient of exactly 0 and a finite loss; an
    estimated point that is nobody's nearest gets only its own term; zero upstream gives exact zeros
  * a second call repeats bit for bit

Before the kernels existed every test here ended at the missing `ops.chamfer_nn` / `ldt_amd.losses`."""
import pytest
import torch

import decoder_train_checks as dc
import kernel_checks as kc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,n,m", dc.CD_SHAPES)
def test_cd_loss_forward_and_backward(B, n, m):
    from ldt_amd import losses, ops
    x1, x2 = dc.cd_case(B, n, m)
    a, b = x1.cuda(), x2.cuda()
    d1, i1, d2, i2 = ops.chamfer_nn(a, b)
    dl, dr = ops.chamfer(a, b)                                           # dl: for every point of b its nearest a; dr: the other way
    assert torch.equal(d1, dr) and torch.equal(d2, dl)
    assert i1.dtype == i2.dtype == torch.int32
    dc.assert_valid_argmin(x1, x2, i1, "idx1")
    dc.assert_valid_argmin(x2, x1, i2, "idx2")
    for type in ("l1", "l2"):
        out = ops.cd_loss(d1, d2, type)
        want = dc.cd_loss_ref(d1.cpu(), d2.cpu(), type)
        r_loss = kc.assert_elementwise(out.cpu(), want, dc.LOSS_REL * want.abs(), "cd_loss %s" % type)
        ref, tol = dc.cd_grad(x1, x2, i1, i2, type, upstream=0.75)
        g = ops.cd_loss_bwd(a, b, i1, i2, type, upstream=0.75)
        r = kc.assert_elementwise(g.cpu(), ref, tol, "cd_loss_bwd %s" % type)
        print("train-kernel cd_loss B%d n%d m%d %s: loss err/tol %.3f, dx1 max err/tol %.3f" % (B, n, m, type, r_loss, r))
        loss, g1 = losses.cd_loss(a, b, type, want_grad=True)
        assert loss.dim() == 0 and float(loss) == float(out[0]) and torch.equal(g1, ops.cd_loss_bwd(a, b, i1, i2, type))
        assert torch.equal(losses.cd_loss(a, b, type), loss)
        assert torch.equal(ops.cd_loss(d1, d2, type), out) and torch.equal(ops.cd_loss_bwd(a, b, i1, i2, type, upstream=0.75), g)   # the same bits
        assert bool((ops.cd_loss_bwd(a, b, i1, i2, type, upstream=0.0) == 0).all())
    again = ops.chamfer_nn(a, b)
    assert all(torch.equal(u, v) for u, v in zip(again, (d1, i1, d2, i2)))


def test_exact_probes():
    from ldt_amd import ops
    # a duplicated target point: the lower index; and the same on the other side
    x1, x2 = dc.cd_case(1, 64, 64)
    was1, was2 = dc.dist_chamfer_torch(x1.double(), x2.double())[2:]
    lo2, lo1 = int(was1.min()), int(was2.min())                          # the lowest target / point that is somebody's nearest
    assert lo1 < 63 and lo2 < 63
    x2[0, 63] = x2[0, lo2]
    x1[0, 63] = x1[0, lo1]
    d1, i1, d2, i2 = ops.chamfer_nn(x1.cuda(), x2.cuda())
    assert not bool((i1 == 63).any()) and not bool((i2 == 63).any())
    keep1, keep2 = (was1 == lo2) & (torch.arange(64) != 63), (was2 == lo1) & (torch.arange(64) != 63)
    assert bool(keep1.any()) and bool(keep2.any())
    assert bool((i1.cpu()[keep1] == lo2).all()) and bool((i2.cpu()[keep2] == lo1).all())
    dc.assert_valid_argmin(x1, x2, i1, "idx1"); dc.assert_valid_argmin(x2, x1, i2, "idx2")
    # a coincident pair: gradient exactly 0 from both terms, finite loss; a far point nobody is nearest to: its own term alone
    x2 = torch.tensor([[[0.0, 0, 0], [1.0, 0, 0], [0.5, 2.0, 0]]])
    x1 = torch.tensor([[[0.25, 0, 0], [1.0, 0, 0], [9.0, 0, 0], [0.5, 2.5, 0]]])
    a, b = x1.cuda(), x2.cuda()
    d1, i1, d2, i2 = ops.chamfer_nn(a, b)
    assert i1.tolist() == [[0, 1, 1, 2]] and i2.tolist() == [[0, 1, 3]] and float(d1[0, 1]) == 0.0 and float(d2[0, 1]) == 0.0
    out = ops.cd_loss(d1, d2, "l1")
    assert bool(out.isfinite().all())
    g = ops.cd_loss_bwd(a, b, i1, i2, "l1").cpu()
    assert g[0, 1].tolist() == [0.0, 0.0, 0.0]
    assert g[0, 2].tolist() == [0.25, 0.0, 0.0]                          # the unit direction over B n = 4, nothing gathered
    assert g[0, 3, 0] == 0 and g[0, 3, 2] == 0 and abs(float(g[0, 3, 1]) - (0.25 + 1.0 / 3)) <= 4 * kc.U24      # its own term and target 2's
    g2 = ops.cd_loss_bwd(a, b, i1, i2, "l2").cpu()
    assert g2[0, 1].tolist() == [0.0, 0.0, 0.0] and g2[0, 2].tolist() == [2 * 8.0 / 4, 0.0, 0.0]
    assert bool(g.isfinite().all()) and bool(g2.isfinite().all())


def test_more_targets_than_one_lds_tile():
    """m past the 2048 indices one LDS tile stages, not a multiple of 4, with several targets per estimated point."""
    from ldt_amd import ops
    x1, x2 = dc.cd_case(1, 37, 4099)
    a, b = x1.cuda(), x2.cuda()
    d1, i1, d2, i2 = ops.chamfer_nn(a, b)
    dc.assert_valid_argmin(x2, x1, i2, "idx2")
    for type in ("l1", "l2"):
        ref, tol = dc.cd_grad(x1, x2, i1, i2, type)
        r = kc.assert_elementwise(ops.cd_loss_bwd(a, b, i1, i2, type).cpu(), ref, tol, "cd_loss_bwd %s, m 4099" % type)
        print("train-kernel cd_loss B1 n37 m4099 %s: dx1 max err/tol %.3f" % (type, r))


def test_refusals_leave_the_device_idle():
    from ldt_amd import ops
    z = torch.zeros(2, 8, 3, device="cuda")
    with pytest.raises(ValueError, match=r"not \[B, n, 3\]"):
        ops.chamfer_nn(z, torch.zeros(3, 8, 3, device="cuda"))
    with pytest.raises(TypeError, match="idx1 must be torch.int32"):
        ops.cd_loss_bwd(z, z, torch.zeros(2, 8, dtype=torch.int64, device="cuda"), torch.zeros(2, 8, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="idx1 .* for x1"):
        ops.cd_loss_bwd(z, z, torch.zeros(2, 4, dtype=torch.int32, device="cuda"), torch.zeros(2, 8, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
